"""ctypes binding of libtce_rvos_train.so (train/tce_rvos_train.h), the training-side sibling of libtce_rvos.so.

One table, loaded lazily: importing the package or calling build_model(args) loads nothing.  The first call of lib() builds the
library if its file is absent (hipcc cross-compiles without a GPU), as smoke() does for the inference library; there is no fallback
path, a failed build raises.
"""
import ctypes as C
import os

HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(HERE, "lib", "libtce_rvos_train.so")

c_f = C.c_void_p  # device pointers travel as integers
i32, i64, f32 = C.c_int32, C.c_int64, C.c_float

MAX_B, MAX_T, MAX_Q, MAX_K = 64, 64, 1024, 128  # TCE_CRIT_MAX_*
MAX_ELEMS = 1 << 30                             # T*h*w of one query


class CriterionConsts(C.Structure):  # tceCriterionConsts
    _fields_ = [("cost_class", f32), ("cost_bbox", f32), ("cost_giou", f32), ("cost_mask", f32), ("cost_dice", f32), ("cost_vis", f32),
                ("focal_alpha", f32)]


# name -> (restype, argtypes): EVERY symbol of train/tce_rvos_train.h and no other (tests/test_criterion_cpu.py checks this)
TRAIN_SIGNATURES = {
    "tce_train_abi_version": (i32, []),
    "tce_train_last_error": (C.c_char_p, []),
    "tce_criterion_mask_sums_ws_bytes": (i64, [i32, i32, i32, i32, i32]),  # B, T, Q, h, w
    # pred [B,T,Q,h,w], tgt [B,T,H,W] u8, sums [B,3,Q] f64, st [B] f64, ws, B, T, Q, h, w, H, W, alpha
    "tce_criterion_mask_sums_f64": (i32, [c_f, c_f, c_f, c_f, c_f, i32, i32, i32, i32, i32, i32, i32, f32, c_f]),
    # logits, pred_boxes, visible | NULL, sums | NULL, st | NULL, labels i64, boxes, valid i32, num_boxes, cost [B,Q], index [B] i32,
    # parts [B,6] f64, losses [6], B, T, Q, K, h, w, consts (host)
    "tce_criterion_match_losses_f32": (i32, [c_f, c_f, c_f, c_f, c_f, c_f, c_f, c_f, c_f, c_f, c_f, c_f, c_f, i32, i32, i32, i32, i32,
                                             i32, C.POINTER(CriterionConsts), c_f]),
    # pred, tgt u8, sums f64, st f64, index i32, num_boxes, gl [6], grad [B,T,Q,h,w], B, T, Q, h, w, H, W, alpha
    "tce_criterion_mask_grad_f32": (i32, [c_f, c_f, c_f, c_f, c_f, c_f, c_f, c_f, i32, i32, i32, i32, i32, i32, i32, f32, c_f]),
    # logits, pred_boxes, visible | NULL, labels i64, boxes, valid i32, index i32, num_boxes, gl [6], g_logits | NULL, g_boxes | NULL,
    # g_visible | NULL, B, T, Q, K, consts (host)
    "tce_criterion_head_grads_f32": (i32, [c_f, c_f, c_f, c_f, c_f, c_f, c_f, c_f, c_f, c_f, c_f, c_f, i32, i32, i32, i32,
                                           C.POINTER(CriterionConsts), c_f]),
}

_LIB = None


class TceTrainError(RuntimeError):
    pass


def lib():
    """Loads the shared object (once), building it first if its file is absent.  No CPU / PyTorch fallback."""
    global _LIB
    if _LIB is None:
        if not os.path.exists(LIB_PATH):
            from . import build as b
            b.build_train(verbose=False)
        l = C.CDLL(LIB_PATH)
        for name, (res, args) in TRAIN_SIGNATURES.items():
            fn = getattr(l, name)  # AttributeError if the symbol is absent
            fn.restype, fn.argtypes = res, args
        _LIB = l
    return _LIB


def check(status, what=""):
    if status != 0:
        msg = lib().tce_train_last_error().decode(errors="replace")
        raise TceTrainError(f"{what} failed ({status}): {msg}")
