"""The resampling rule of include/gdlhip_raster.h restated in float64 numpy, the yardstick of tests/test_raster_host.py and
tests/test_hip_raster.py.  It shares no code with the library.

Destination pixel (y, x) lies at u = (x + 0.5) sx + ox, v = (y + 0.5) sy + oy of the source.  Per axis with centre c, scale s and
source size n: f = max(1, s), support R f (R = 1 bilinear, 2 cubic: Catmull-Rom, a = -0.5), taps k in [max(0, floor(c - R f +
0.5)), min(n, floor(c + R f + 0.5))) with weight K((k + 0.5 - c) / f).  A sample equal to its band's nodata is masked (NaN nodata:
a NaN sample).  Value = sum(wy wx m v) / sum(wy wx m); valid iff the sample that contains (u, v) exists and is unmasked and
sum(w m) >= 0.25 sum(w), sum(w) over the taps inside the source.  Nearest: the sample at (floor(u), floor(v))."""

from typing import NamedTuple

import numpy as np

MIN_VALID_WEIGHT = 0.25
RADIUS = {"bilinear": 1.0, "cubic": 2.0}
INT_RANGE = {np.dtype(np.uint8): (0, 255), np.dtype(np.uint16): (0, 65535), np.dtype(np.int16): (-32768, 32767)}


class Warp(NamedTuple):      # of one band; every field [Hd, Wd]
    num: np.ndarray          # sum wy wx m v (float64)
    den: np.ndarray          # sum wy wx m
    tot: np.ndarray          # sum wy wx over the taps inside the source
    valid: np.ndarray        # bool
    taps: np.ndarray         # T: the number of taps (rows x columns)
    spread: np.ndarray       # S: sum |wy wx m v| / sum wy wx m (inf where that is not positive)


def kernel(t: np.ndarray, method: str) -> np.ndarray:
    t = np.abs(np.asarray(t, dtype=np.float64))
    if method == "bilinear":
        return np.where(t < 1.0, 1.0 - t, 0.0)
    near = (1.5 * t - 2.5) * t * t + 1.0
    far = ((-0.5 * t + 2.5) * t - 4.0) * t + 2.0
    return np.where(t < 1.0, near, np.where(t < 2.0, far, 0.0))


def centres(n_dst: int, s: float, o: float) -> np.ndarray:
    return (np.arange(n_dst, dtype=np.float64) + 0.5) * np.float64(s) + np.float64(o)


def axis_taps(n_dst: int, n_src: int, s: float, o: float, method: str) -> tuple[np.ndarray, np.ndarray]:
    """(weights float64 [n_dst, n_src], 0 outside the taps; taps bool [n_dst, n_src]) of one axis."""
    f = max(1.0, float(s))
    support = RADIUS[method] * f
    c = centres(n_dst, s, o)
    lo = np.minimum(np.maximum(np.floor(c - support + 0.5), 0.0), n_src)
    hi = np.minimum(np.maximum(np.floor(c + support + 0.5), 0.0), n_src)
    k = np.arange(n_src, dtype=np.float64)
    taps = (k[None, :] >= lo[:, None]) & (k[None, :] < hi[:, None])
    return np.where(taps, kernel((k[None, :] + 0.5 - c[:, None]) / f, method), 0.0), taps


def masked(band: np.ndarray, nodata) -> np.ndarray:
    """bool [H, W]: the samples of the band that are nodata."""
    if nodata is None:
        return np.zeros(band.shape, dtype=bool)
    return np.isnan(band) if nodata != nodata else band.astype(np.float64) == np.float64(nodata)


def centre_valid(band: np.ndarray, Hd: int, Wd: int, sx, ox, sy, oy, nodata) -> tuple[np.ndarray, np.ndarray, np.ndarray]:
    """(ok [Hd, Wd], row index [Hd], column index [Wd]) of the sample that contains each destination centre."""
    H, W = band.shape
    u, v = centres(Wd, sx, ox), centres(Hd, sy, oy)
    inx, iny = (u >= 0) & (u < W), (v >= 0) & (v < H)
    ix = np.where(inx, np.floor(u), 0).astype(np.int64)
    iy = np.where(iny, np.floor(v), 0).astype(np.int64)
    ok = iny[:, None] & inx[None, :] & ~masked(band, nodata)[iy[:, None], ix[None, :]]
    return ok, iy, ix


def warp_band(band: np.ndarray, Hd: int, Wd: int, sx, ox, sy, oy, method: str, nodata=None) -> Warp:
    """The sums of one band [H, W] for bilinear or cubic: each is separable, so a product of the two axes' weight matrices with
    the band (a NaN sample that is not masked makes the sums of the pixels whose taps hold it NaN, as the plain sum would)."""
    H, W = band.shape
    m = (~masked(band, nodata)).astype(np.float64)
    v = np.where(m > 0, band.astype(np.float64), 0.0)
    bad = np.isnan(v)
    v = np.where(bad, 0.0, v)
    (wx, inx), (wy, iny) = axis_taps(Wd, W, sx, ox, method), axis_taps(Hd, H, sy, oy, method)
    num, den = wy @ (m * v) @ wx.T, wy @ m @ wx.T
    num = np.where(iny.astype(np.float64) @ bad @ inx.T.astype(np.float64) > 0, np.nan, num)
    tot = wy.sum(axis=1)[:, None] * wx.sum(axis=1)[None, :]
    taps = iny.sum(axis=1)[:, None] * inx.sum(axis=1)[None, :]
    spread = np.abs(wy) @ np.abs(m * v) @ np.abs(wx).T
    ok, _, _ = centre_valid(band, Hd, Wd, sx, ox, sy, oy, nodata)
    valid = ok & (den >= MIN_VALID_WEIGHT * tot)
    with np.errstate(divide="ignore", invalid="ignore"):
        spread = np.where(den > 0, spread / den, np.inf)
    return Warp(num, den, tot, valid, taps, spread)


def warp(src: np.ndarray, dst_shape, sx, ox, sy, oy, method: str, nodata=None, dst_nodata=0, out_dtype=None):
    """(dst [C, Hd, Wd] of out_dtype, valid uint8 [C, Hd, Wd], [Warp per band] or None for nearest): what ops.raster_warp returns,
    the division in float64 (an integer destination: floor(q + 0.5), clamped).  nodata: None, a number or a list per band."""
    Cc, (Hd, Wd) = src.shape[0], dst_shape
    out_dtype = np.dtype(src.dtype if out_dtype is None else out_dtype)
    per_band = list(nodata) if isinstance(nodata, (list, tuple)) else [nodata] * Cc
    dst = np.full((Cc, Hd, Wd), dst_nodata, dtype=out_dtype)
    valid = np.zeros((Cc, Hd, Wd), dtype=np.uint8)
    sums = []
    for c in range(Cc):
        if method == "nearest":
            ok, iy, ix = centre_valid(src[c], Hd, Wd, sx, ox, sy, oy, per_band[c])
            value = src[c][iy[:, None], ix[None, :]].astype(np.float64)
        else:
            s = warp_band(src[c], Hd, Wd, sx, ox, sy, oy, method, per_band[c])
            sums.append(s)
            ok = s.valid
            with np.errstate(divide="ignore", invalid="ignore"):
                value = s.num / s.den
            if out_dtype in INT_RANGE:
                value = np.clip(np.floor(np.where(ok, value, 0.0) + 0.5), *INT_RANGE[out_dtype])
        dst[c][ok] = value[ok].astype(out_dtype)
        valid[c] = ok
    return dst, valid, (sums or None)
