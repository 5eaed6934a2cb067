"""Outpainting restated in numpy, integers and fp64, from the text of include/arcflow_hip.h and of ``schedule.outpaint_plan``'s docstring: the
index rules of the two fills, the canvas and its mask (afx_canvas_extend), the mark of a window (afx_canvas_mark) and the host replay of
the mask state over a list of windows.  Written with explicit index arithmetic, no ``np.pad``: the tests hold the rules against it."""
import numpy as np

FAR = np.iinfo(np.int64).max // 4          # the distance of a pixel that no counted side bounds


def edge_index(i, n):
    return np.clip(np.asarray(i, dtype=np.int64), 0, n - 1)


def reflect_index(i, n):
    i = np.asarray(i, dtype=np.int64)
    if n == 1:
        return np.zeros_like(i)
    p = 2 * (n - 1)
    j = ((i % p) + p) % p
    return np.where(j < n, j, p - j)


def src_index(i, n, fill):
    return {'edge': edge_index, 'reflect': reflect_index}[fill](i, n)


def ramp(d, blend):
    """max(0, 1 - (d + 1) / (blend + 1)) in fp64; 0 at the distance FAR."""
    d = np.asarray(d, dtype=np.int64)
    r = np.maximum(0.0, 1.0 - (d + 1).astype(np.float64) / np.float64(blend + 1))
    return np.where(d >= FAR, 0.0, r)


def side_distance(n, lo, hi):
    """[n] int64: the distance of pixel i to the nearest counted side of an axis of n pixels (``lo``: the side at 0 counts, ``hi``: the one
    at n - 1); FAR where neither counts."""
    i = np.arange(n, dtype=np.int64)
    d = np.full(n, FAR, dtype=np.int64)
    if lo:
        d = np.minimum(d, i)
    if hi:
        d = np.minimum(d, n - 1 - i)
    return d


def rect_ramp(h, w, top, bottom, left, right, blend):
    """[h, w] fp64: ramp of the distance to the nearest counted side of an h x w rectangle."""
    d = np.minimum(side_distance(h, top, bottom)[:, None], side_distance(w, left, right)[None, :])
    return ramp(d, blend)


def canvas_extend(src, left, top, right, bottom, fill, blend):
    """src uint8 [B, H, W, 3] -> (canvas uint8 [B, Hc, Wc, 3], mask fp64 [Hc, Wc])."""
    B, H, W, _ = src.shape
    Hc, Wc = H + top + bottom, W + left + right
    iy = src_index(np.arange(Hc) - top, H, fill)
    ix = src_index(np.arange(Wc) - left, W, fill)
    canvas = src[:, iy[:, None], ix[None, :], :]
    mask = np.ones((Hc, Wc), dtype=np.float64)
    mask[top:top + H, left:left + W] = rect_ramp(H, W, top > 0, bottom > 0, left > 0, right > 0, blend)
    return canvas, mask


def canvas_mark(M, window, blend):
    """A copy of M [Hc, Wc] with min(M, ramp(d)) on the window, d to the nearest window side that is not on the canvas border."""
    Hc, Wc = M.shape
    x0, y0, x1, y1 = window
    out = M.copy()
    r = rect_ramp(y1 - y0, x1 - x0, y0 > 0, y1 < Hc, x0 > 0, x1 < Wc, blend)
    out[y0:y1, x0:x1] = np.minimum(out[y0:y1, x0:x1], r.astype(M.dtype))
    return out


def replay(H, W, left, top, right, bottom, blend, windows):
    """The mask state over ``windows`` in order -> (M at the end, [whether window k held a pixel with M > 0 at its turn])."""
    _, M = canvas_extend(np.zeros((1, H, W, 3), dtype=np.uint8), left, top, right, bottom, 'edge', blend)
    live = []
    for win in windows:
        x0, y0, x1, y1 = win
        live.append(bool((M[y0:y1, x0:x1] > 0).any()))
        M = canvas_mark(M, win, blend)
    return M, live
