"""The yardstick of tests/test_gpu_frames.py: the statements of the reference's run_nerf.py that turn float32 frames into 8-bit pictures,
written on NumPy float32 arrays with their line numbers -- NumPy itself, executed, so there is no tolerance to choose.  The OpenCV call
cv2.applyColorMap(255 - g, table) is the lookup lut[255 - g] in the caller's [256, 3] table.

Two stated deviations, where the reference's result is undefined:
  * a slice whose divisor is 0 -- maximum 0, or maximum == minimum in the video form -- is grey level 0 throughout (the reference divides
    by zero: NaN or inf cast to uint8);
  * a NaN value is grey level 0 (NaN cast to uint8 is undefined) and takes no part in a minimum or maximum: np.nanmax / np.nanmin, which
    equal .max() / .min() on data without NaN.
checked, with the float32 operation order of np.mean(-1), by tests/test_frames_ref.py."""
import numpy as np


def to8b(x):
    """utils/misc.py:6, with NaN -> 0"""
    x = np.asarray(x, np.float32)
    return (255 * np.clip(np.where(np.isnan(x), np.float32(0), x), 0, 1)).astype(np.uint8)


def pixmse(rgb, gtrgb):
    """run_nerf.py:670"""
    return ((rgb - gtrgb) ** 2).mean(-1)


def mean3_explicit(a):
    """what np.mean(-1) of a float32 [..., 3] array does: ((a0 + a1) + a2) / float32(3), each step rounded to float32"""
    a = np.asarray(a, np.float32)
    return ((a[..., 0] + a[..., 1]) + a[..., 2]) / np.float32(3)


def _over_max(v, mx):
    """to8b(v / float(mx)), the form of :382, :389, :675, :679, :732; maximum 0: grey level 0"""
    if float(mx) == 0.0:
        return np.zeros(v.shape, np.uint8)
    return to8b(v / float(mx))


def _pick(g, lut):
    return g if lut is None else np.asarray(lut, np.uint8)[255 - g]          # cv2.applyColorMap(255 - g, table), :385, :675, :679


def depth_images(disps, invert=True, scope="all", lut=None):
    """invert: disps = 1. - disps (:374, :663).  scope 'all': to8b(disp / float(disps.max())) (:389, :675, :732); scope 'frame':
    to8b(disps[i] / disps[i].max()) (:382).  With a table: the colour map on 255 - that (:385, :675)."""
    d = np.asarray(disps, np.float32)
    if invert:
        d = np.float32(1.) - d
    with np.errstate(all="ignore"):
        if scope == "all":
            g = _over_max(d, np.nanmax(d))
        else:
            g = np.stack([_over_max(f, np.nanmax(f)) for f in d])
    return _pick(g, lut)


def error_maps(rgbs, gts, lut=None):
    """per frame: pixmse = ((rgb - gtrgb) ** 2).mean(-1) (:670), to8b(pixmse / float(pixmse.max())) (:679), the colour map on 255 - that"""
    out = []
    with np.errstate(all="ignore"):
        for rgb, gt in zip(np.asarray(rgbs, np.float32), np.asarray(gts, np.float32)):
            e = pixmse(rgb, gt)
            out.append(_over_max(e, np.nanmax(e)))
    return _pick(np.stack(out), lut)


def video_frames(rgbs):
    """rgbs = (rgbs - rgbs.min()) / (rgbs.max() - rgbs.min()) (:726), to8b(rgbs) (:730); maximum == minimum: grey level 0"""
    x = np.asarray(rgbs, np.float32)
    with np.errstate(all="ignore"):
        mn, mx = np.nanmin(x), np.nanmax(x)
        if mx == mn:
            return np.zeros(x.shape, np.uint8)
        return to8b((x - mn) / (mx - mn))
