"""The three rules of include/gdlhip_raster_tone.h restated in numpy float64: what the GPU tests compare with, bit for bit.
Rasters are numpy [C, H, W]; ``nodata`` is None, one number or one entry per band (None for a band without)."""

import numpy as np

LAYOUT = {np.dtype(np.uint8): (256, 0.0), np.dtype(np.uint16): (65536, 0.0), np.dtype(np.int16): (65536, -32768.0)}      # bins, value of bin 0


def band_nodata(nodata, channels):
    return list(nodata) if isinstance(nodata, (list, tuple)) else [nodata] * channels


def masked(band, nd):
    """True where a sample is its band's nodata (a NaN nodata: where the sample is NaN)."""
    if nd is None:
        return np.zeros(band.shape, dtype=bool)
    return np.isnan(band) if nd != nd else band == band.dtype.type(nd)


def hist(src, nodata=None, bins=None, value_range=None):
    """int64 [C, bins + 2]: the bins, then under and over."""
    C = src.shape[0]
    nds = band_nodata(nodata, C)
    if src.dtype in LAYOUT:
        bins, origin = LAYOUT[src.dtype]
        out = np.zeros((C, bins + 2), dtype=np.int64)
        for c in range(C):
            live = src[c][~masked(src[c], nds[c])]
            out[c, :bins] = np.bincount(live.astype(np.int64) - int(origin), minlength=bins)
        return out
    ranges = [value_range] * C if np.ndim(value_range) == 1 else list(value_range)
    out = np.zeros((C, bins + 2), dtype=np.int64)
    for c in range(C):
        lo, hi = (np.float64(v) for v in ranges[c])
        v = src[c][~masked(src[c], nds[c])].astype(np.float64)
        v = v[~np.isnan(v)]
        inside = v[(v >= lo) & (v <= hi)]
        b = np.minimum(np.floor((inside - lo) / (hi - lo) * np.float64(bins)), bins - 1).astype(np.int64)
        out[c, :bins] = np.bincount(b, minlength=bins)
        out[c, bins], out[c, bins + 1] = (v < lo).sum(), (v > hi).sum()
    return out


def quantiles(acc, bins, qs, origin, step):
    """float64 [C, Q] from the bin words of ``acc`` [C, bins + 2]."""
    out = np.full((acc.shape[0], len(qs)), np.nan)
    for c in range(acc.shape[0]):
        cum = np.cumsum(acc[c, :bins])
        N = int(cum[-1])
        if N == 0:
            continue
        for j, q in enumerate(qs):
            r = int(np.floor(np.float64(q) * np.float64(N - 1)))
            b = int(np.searchsorted(cum, r, side="right"))      # the smallest bin whose inclusive count exceeds r
            out[c, j] = np.float64(origin[c]) + np.float64(b) * np.float64(step[c])
    return out


def edges(dtype, channels, bins=None, value_range=None):
    """(bins, origin, step) as the Python layer passes them."""
    if np.dtype(dtype) in LAYOUT:
        bins, origin = LAYOUT[np.dtype(dtype)]
        return bins, [origin] * channels, [1.0] * channels
    ranges = [value_range] * channels if np.ndim(value_range) == 1 else list(value_range)
    return bins, [float(lo) for lo, _ in ranges], [(float(hi) - float(lo)) / bins for lo, hi in ranges]


def stretch(src, bounds, out_range=(0, 255), nodata=None, dst_nodata=0, out_dtype=np.uint8):
    """(dst, valid): [C, H, W] of ``out_dtype`` (uint8 or float32) and the uint8 validity planes."""
    C = src.shape[0]
    nds = band_nodata(nodata, C)
    out_lo, out_hi = np.float64(out_range[0]), np.float64(out_range[1])
    dst = np.empty(src.shape, dtype=out_dtype)
    valid = np.empty(src.shape, dtype=np.uint8)
    with np.errstate(all="ignore"):
        for c in range(C):
            lo, hi = np.float64(bounds[c][0]), np.float64(bounds[c][1])
            v = src[c].astype(np.float64)
            dead = not (np.isfinite(lo) and np.isfinite(hi) and np.isfinite(hi - lo))
            bad = masked(src[c], nds[c]) | np.isnan(v) | dead
            v = np.where(bad, 0.0, v)
            t = np.where(v > lo, 1.0, 0.0) if dead or hi <= lo else np.clip((v - lo) / (hi - lo), 0.0, 1.0)
            y = out_lo + t * (out_hi - out_lo)
            if np.dtype(out_dtype) == np.uint8:
                res = np.clip(np.floor(y + 0.5), 0.0, 255.0).astype(np.uint8)
            else:
                res = y.astype(np.float32)
            dst[c] = np.where(bad, np.dtype(out_dtype).type(dst_nodata), res)
            valid[c] = ~bad
    return dst, valid
