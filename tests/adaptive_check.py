"""A numpy restatement of the adaptive sampling rule (include/skr.h skr_render_adaptive) in explicit binary32
operations: the expected passes, means and bytes of any sequence of float frames."""
import numpy as np

from denoise_check import quantise

f32 = np.float32
LUM_FLOOR = f32(0.00390625)  # include/skr.h SKR_ADAPTIVE_LUM_FLOOR (2^-8)


def lum(v):
    """l = 0.2126f * r + 0.7152f * g + 0.0722f * b, left to right, of v [..., 3]"""
    v = np.asarray(v, np.float32)
    return ((f32(0.2126) * v[..., 0] + f32(0.7152) * v[..., 1]) + f32(0.0722) * v[..., 2]).astype(np.float32)


def converged(S1, S2, n, threshold):
    """e2 <= b * b after n passes (only asked where the rule runs the test)"""
    with np.errstate(invalid="ignore", divide="ignore", over="ignore"):
        nf = f32(n)
        m = (S1 / nf).astype(np.float32)
        d = (S2 / nf - m * m).astype(np.float32)
        var = np.where(d > 0, d, f32(0)).astype(np.float32)
        e2 = (var / (nf - f32(1))).astype(np.float32)
        b = (f32(threshold) * np.where(m > LUM_FLOOR, m, LUM_FLOOR)).astype(np.float32)
        return e2 <= b * b


def adaptive(frame, min_passes, max_passes, threshold):
    """frame(k) -> float32 [N, 3], the frame of pass k (seed + k).  Returns (mean float32 [N, 3], bytes uint8 [N, 3], passes uint32 [N]);
    frame(k) is asked only for the passes some pixel gets."""
    assert 1 <= min_passes <= max_passes and not np.isnan(threshold)
    v = np.asarray(frame(0), np.float32).reshape(-1, 3)
    C = v.copy()
    l = lum(v)
    S1, S2 = l.copy(), (l * l).astype(np.float32)
    n = np.ones(len(v), np.uint32)
    active = np.ones(len(v), bool)
    with np.errstate(invalid="ignore", over="ignore"):
        for k in range(1, max_passes):
            if k >= min_passes and k >= 2 and threshold >= 0:
                active &= ~converged(S1, S2, k, threshold)
            if not active.any():
                break
            v = np.asarray(frame(k), np.float32).reshape(-1, 3)
            l = lum(v)
            C[active] = C[active] + v[active]
            S1[active] = S1[active] + l[active]
            S2[active] = S2[active] + (l * l).astype(np.float32)[active]
            n[active] += 1
        mean = (C / n.astype(np.float32)[:, None]).astype(np.float32)
    return mean, quantise(mean), n
