"""The sample rule of the dense-field operators (include/dfe.h: dfe_fill_holes_f32, dfe_weighted_median_f32, dfe_guided_upsample_f32;
csrc/dfe_field.h on the device) stated once in numpy, for their restatements (tests/fill_ref64.py, wmedian_ref.py, upsample_ref.py).
A helper, no tests."""
import numpy as np

F = np.float32
W_MIN = F(1e-6)   # the fp32 constant of the definition: a weight below it is a hole


def validity(v, w):
    """a [H][W] float32 for values v [C][H][W] and weights w [H][W]: min(w, 1) where w is finite, w >= 1e-6f and every channel of v is
    finite, else 0; w None: ones"""
    v = np.asarray(v, F)
    w = np.ones(v.shape[1:], F) if w is None else np.asarray(w, F)
    with np.errstate(invalid="ignore"):
        ok = np.isfinite(w) & (w >= W_MIN) & np.isfinite(v).all(axis=0)
        return np.where(ok, np.minimum(w, F(1)), F(0)).astype(F)
