"""fp64 numpy restatement of the table-driven separable resampling (afx_image_resample) and an independent statement of the table rule.

``resample`` consumes the SAME fp32 tables the kernel gets (start, count, w[n_out, taps]), widened to fp64, so what it measures is the
kernel's arithmetic alone: two fp32 dot products per element, the uint8 conversion and the clamp.  Per element it also returns
    bound = 2^-24 (taps_h + taps_v + 4) sum_v |w_v| sum_h |w_h| |x|
(taps = the tables' row strides).  Where it comes from: an fp32 dot product of n terms by fma is off by at most n 2^-24 sum |w||x| (to first
order); the horizontal pass contributes taps_h of these units, carried through the vertical weights, the vertical pass taps_v on the
horizontal sums; the uint8 quotient x / 255 is one more rounding of x, and the clamp is 1-Lipschitz.  That is taps_h + taps_v + 1; the
remaining 3 units cover every second-order term.

``rule_table`` / ``gaussian_rule`` state the rule of the C function in plain Python floats (fp64), with switches that turn it into the
mutants the kernel test must reject.
"""
import math

import numpy as np

A = {'lanczos3': 3.0, 'triangle': 1.0}


def _sinc(x):
    if x == 0.0:
        return 1.0
    if x == math.floor(x):          # the exact zeros of sin(pi x) / (pi x)
        return 0.0
    return math.sin(math.pi * x) / (math.pi * x)


def _f(name, x):
    if name == 'lanczos3':
        return _sinc(x) * _sinc(x / 3.0) if -3.0 <= x < 3.0 else 0.0
    return max(0.0, 1.0 - abs(x))


def _pack(rows, n_out):
    taps = max(len(r[1]) for r in rows)
    start = np.array([r[0] for r in rows], dtype=np.int32)
    count = np.array([len(r[1]) for r in rows], dtype=np.int32)
    w = np.zeros((n_out, taps), dtype=np.float64)
    for i, r in enumerate(rows):
        w[i, :len(r[1])] = r[1]
    return start, count, w


def rule_table(n_in, n_out, name='lanczos3', box=None, normalise=True, fs_one=False, shift=0):
    """Pillow's Image.resize(..., box=) along one axis -> (start int32, count int32, w float64 [n_out, taps]).
    normalise=False, fs_one=True (the filter is not widened on a downscale) and shift (the window starts ``shift`` pixels late) are mutants."""
    b0, b1 = (0.0, float(n_in)) if box is None else box
    scale = (b1 - b0) / n_out
    fs = 1.0 if fs_one else max(scale, 1.0)
    support = A[name] * fs
    rows = []
    for i in range(n_out):
        c = b0 + (i + 0.5) * scale
        lo = max(0, int(c - support + 0.5))
        hi = min(n_in, int(c + support + 0.5))
        ws = [_f(name, (k + lo - c + 0.5) / fs) for k in range(hi - lo)]
        tot = sum(ws) if normalise else 1.0
        lo = min(lo + shift, n_in - len(ws))
        rows.append((lo, [v / tot for v in ws]))
    return _pack(rows, n_out)


def gaussian_rule(n, sigma):
    r = int(math.ceil(3.0 * sigma))
    rows = []
    for i in range(n):
        lo, hi = max(0, i - r), min(n, i + r + 1)
        ws = [math.exp(-float(k - i) ** 2 / (2.0 * sigma * sigma)) for k in range(lo, hi)]
        rows.append((lo, [v / sum(ws) for v in ws]))
    return _pack(rows, n)


def dense(table, n_in):
    """The [n_out, n_in] fp64 matrix of a table (weights widened exactly)."""
    start, count, w = (np.asarray(t) for t in table)
    m = np.zeros((len(start), n_in), dtype=np.float64)
    for i in range(len(start)):
        for k in range(int(count[i])):
            m[i, min(max(int(start[i]) + k, 0), n_in - 1)] += float(w[i, k])
    return m


def to_planar01(src):
    """uint8 [B, H, W, C] -> fp64 [B, C, H, W] as x / 255 (exact quotient in fp64); an fp32 [B, C, H, W] source is widened."""
    src = np.asarray(src)
    if src.dtype == np.uint8:
        return src.astype(np.float64).transpose(0, 3, 1, 2) / 255.0
    return src.astype(np.float64)


def resample(src, tab_h, tab_w, clamp=True):
    """-> (out, bound), both fp64 [B, C, H_out, W_out]: the horizontal pass with ``tab_w``, then the vertical pass with ``tab_h``."""
    x = to_planar01(src)
    mh, mw = dense(tab_h, x.shape[2]), dense(tab_w, x.shape[3])
    out = np.einsum('yh,bchw,xw->bcyx', mh, x, mw, optimize=True)
    mag = np.einsum('yh,bchw,xw->bcyx', np.abs(mh), np.abs(x), np.abs(mw), optimize=True)
    units = np.asarray(tab_h[2]).shape[1] + np.asarray(tab_w[2]).shape[1] + 4
    if clamp:
        out = np.clip(out, 0.0, 1.0)
    return out, 2.0 ** -24 * units * mag
