"""Time grid of the ArcFlow sampler and the flow-matching scheduler object the reference's entry
scripts configure (inference_flux.py:14-15: ``FlowMatchEulerDiscreteScheduler.from_config(
pipe.scheduler.config, shift=3.2, shift_terminal=None, use_dynamic_shifting=False)``), and the
``FlowEulerODEScheduler`` of the reference's own teacher sampling (GaussianFlow.forward_test).

Host-side float arithmetic only (128 numbers per image) -- nothing here runs on the GPU.
"""
from __future__ import annotations

import math
from typing import Any, Dict, List, NamedTuple, Optional, Tuple

import numpy as np
import torch


def retrieve_raw_timesteps(num_inference_steps: int, total_substeps: int, timestep_ratio: float
                           ) -> Tuple[List[float], List[int], int]:
    """Raw sub-step times, sub-steps per inference step and their total
    (same contract as lakonlab/pipelines/arcflux_pipeline.py:34-70)."""
    if num_inference_steps < 1:
        raise ValueError('num_inference_steps must be >= 1')
    seg = 1.0 / (num_inference_steps - 1 + timestep_ratio)
    times: List[float] = []
    per_step: List[int] = []
    upper = 1.0
    for i in range(num_inference_steps):
        size = seg * timestep_ratio if i == num_inference_steps - 1 else seg
        n = max(round(size * total_substeps), 1)
        per_step.append(n)
        times += np.linspace(upper, upper - size, n, endpoint=False).clip(min=0.0).tolist()
        upper -= size
    return times, per_step, sum(per_step)


def edit_raw_timesteps(num_inference_steps: int, total_substeps: int, timestep_ratio: float, strength: float
                       ) -> Tuple[List[float], List[int], int]:
    """The raw grid of an edit (``image=`` / ``strength=`` on the pipelines): ``retrieve_raw_timesteps`` with every time multiplied by
    ``strength`` in (0, 1].  The edit takes ``num_inference_steps`` full student steps over the raw time [strength, 0]; it does not walk a
    truncated prefix of the text-to-image grid, which at 2 NFE could only express strength 0.5 or 1.  strength == 1.0 returns the lists of
    ``retrieve_raw_timesteps`` themselves."""
    strength = float(strength)
    if not 0.0 < strength <= 1.0:
        raise ValueError(f'strength must be in (0, 1], got {strength}')
    times, per_step, total = retrieve_raw_timesteps(num_inference_steps, total_substeps, timestep_ratio)
    if strength != 1.0:
        times = [strength * t for t in times]
    return times, per_step, total


def truncate_by_strength(sigmas: torch.Tensor, strength: float) -> Tuple[int, torch.Tensor]:
    """The schedule of a many-step edit (``sample_teacher(image=..., strength=...)``, TeacherSampler with ``x0``): a suffix of the
    sampler's FULL schedule ``sigmas`` [n + 1] (trailing 0; shift / dynamic shifting already applied for all n steps), as the
    image-to-image pipelines of diffusers truncate theirs (as recalled; unpinned):

        init = min(n * strength, n),   t_start = int(max(n - init, 0)),   steps t_start .. n - 1 run

    -> (t_start, sigmas[t_start:]): the edit starts from the source noised to ``sigmas[t_start]``.  ``strength`` must lie in (0, 1];
    1.0 keeps all n steps, and a strength so small that no step is left raises like one outside the interval."""
    strength = float(strength)
    if not 0.0 < strength <= 1.0:
        raise ValueError(f'strength must be in (0, 1], got {strength}')
    n = int(sigmas.numel()) - 1
    if n < 1:
        raise ValueError('sigmas: need at least one step (two entries)')
    t_start = int(max(n - min(n * strength, n), 0))
    if t_start >= n:
        raise ValueError(f'strength {strength} leaves none of the {n} steps to run')
    return t_start, sigmas[t_start:]


def mask_to_tokens(mask: torch.Tensor, hp: int, wp: int, reduce: str = 'max') -> torch.Tensor:
    """An image-resolution mask [B, 1, H, W] or [B, H, W] with H = 16 hp, W = 16 wp -> [B, hp*wp, 4] fp32, the operand of
    ``ops.edit_blend``: latent pixel (2r + ph, 2c + pw) of token r*wp + c, at index ph*2 + pw, takes the max (``reduce='max'``: any
    repainted pixel repaints its latent pixel, a binary mask stays binary) or the mean (``'mean'``) of its 8 x 8 pixel block.  Once per
    call, on whatever device the mask lives: plain torch."""
    if reduce not in ('max', 'mean'):
        raise ValueError(f"reduce: 'max' or 'mean', got {reduce!r}")
    if mask.dim() == 4 and mask.shape[1] == 1:
        mask = mask[:, 0]
    if mask.dim() != 3 or tuple(mask.shape[1:]) != (16 * hp, 16 * wp):
        raise ValueError(f'mask: need [B, 1, {16 * hp}, {16 * wp}] or [B, {16 * hp}, {16 * wp}], got {tuple(mask.shape)}')
    blocks = mask.to(torch.float32).reshape(mask.shape[0], hp, 2, 8, wp, 2, 8)          # [B, r, ph, i, c, pw, j]
    red = blocks.amax(dim=(3, 6)) if reduce == 'max' else blocks.mean(dim=(3, 6))      # [B, r, ph, c, pw]
    return red.permute(0, 1, 3, 2, 4).reshape(mask.shape[0], hp * wp, 4).contiguous()


def mask_crop_window(bbox, src_h: int, src_w: int, height: int, width: int, pad: int) -> Tuple[int, int, int, int]:
    """The window (x0, y0, x1, y1) of a ``src_h`` x ``src_w`` image that an edit with ``padding_mask_crop=pad`` works on, from the mask's
    half-open bounding box ``bbox`` = (x0, y0, x1, y1) (``ops.mask_bbox``) and the call's ``height`` x ``width``.  Host integer arithmetic:
    the box is padded by ``pad`` pixels on each side and clipped to the image; then the shorter side (measured against the call's aspect
    ratio) grows to ``want = min(side of the image, ceil(other side * aspect))``, half of the growth on either side, shifted back inside
    where that would cross a border.  The window always contains the padded box and lies inside the image.  It has the call's aspect
    ratio up to the integer rounding UNLESS the image is too small for it (``want`` was cut to the image's side): the resample to the
    call's size then stretches.  An empty box (no mask pixel > 0: ``x1 <= x0`` or ``y1 <= y0``) raises ValueError."""
    x0, y0, x1, y1 = (int(v) for v in bbox)
    H, W, pad = int(src_h), int(src_w), int(pad)
    if x1 <= x0 or y1 <= y0:
        raise ValueError(f'the mask has no pixel > 0 (bounding box {(x0, y0, x1, y1)}): `padding_mask_crop` has nothing to crop to')
    if pad < 0 or height < 1 or width < 1 or x0 < 0 or y0 < 0 or x1 > W or y1 > H:
        raise ValueError(f'need pad >= 0, height, width >= 1 and a box inside the {H} x {W} image, got box {(x0, y0, x1, y1)}, pad {pad}, '
                         f'{height} x {width}')
    x0, y0, x1, y1 = max(x0 - pad, 0), max(y0 - pad, 0), min(x1 + pad, W), min(y1 + pad, H)
    cw, ch = x1 - x0, y1 - y0
    if cw * height < ch * width:            # narrower than the call: widen
        want = min(W, -(-ch * width // height))
        x0 = min(max(x0 - (want - cw) // 2, 0), W - want)
        x1 = x0 + want
    else:                                   # heighten (want == ch when the aspect is the call's already)
        want = min(H, -(-cw * height // width))
        y0 = min(max(y0 - (want - ch) // 2, 0), H - want)
        y1 = y0 + want
    return x0, y0, x1, y1


AFX_TILE_MAX_TAPS = 4          # arcflow_hip.h: the most tiles that may cover one pixel along an axis


def tile_axis_weights(L: int, t: int, origins) -> Tuple[np.ndarray, np.ndarray, np.ndarray]:
    """The cross-fade of tiles of side ``t`` at ``origins`` (strictly increasing, first 0, last L - t, no gap) along an axis of ``L``
    pixels, in fp64: -> (start [L] int32, count [L] int32, w [L, max(count)] float64, zero padded).  Tile i weighs pixel x of its span
    with u_i(x) = min(x - o_i + 1 if i > 0 else inf, o_i + t - x if i < k - 1 else inf) (1 when both are infinite: a single tile), a ramp
    that rises from 1 at an inner edge, and w_i(x) = u_i(x) / sum_j u_j(x): a linear cross-fade over whatever the overlap is, full weight
    on the canvas borders, a partition of unity everywhere.  The tiles covering x are consecutive: start[x] .. start[x] + count[x] - 1."""
    o = np.asarray(origins, dtype=np.int64)
    k = int(o.size)
    x = np.arange(L, dtype=np.int64)
    first = np.searchsorted(o + t, x, side='right')            # the first tile with o_i + t > x
    last = np.searchsorted(o, x, side='right') - 1             # the last tile with o_i <= x
    count = last - first + 1
    if k < 1 or o[0] != 0 or o[-1] != L - t or (count < 1).any():
        raise ValueError(f'origins {o.tolist()} with tile side {t} do not cover [0, {L})')
    taps = int(count.max())
    w = np.zeros((L, taps), dtype=np.float64)
    for a in range(taps):
        i = np.minimum(first + a, k - 1)
        dl = np.where(i > 0, x - o[i] + 1, np.inf)
        dr = np.where(i < k - 1, o[i] + t - x, np.inf)
        u = np.minimum(dl, dr)
        w[:, a] = np.where(a < count, np.where(np.isinf(u), 1.0, u), 0.0)
    w /= w.sum(axis=1, keepdims=True)
    return first.astype(np.int32), count.astype(np.int32), w


def tile_axis(L: int, tile: int, overlap: int) -> Tuple[int, np.ndarray, np.ndarray, np.ndarray, np.ndarray]:
    """The tile plan of one axis of ``L`` canvas pixels (``pipe.enhance``): -> (t, origins [k] int32, start [L] int32, count [L] int32,
    w [L, taps] float32), the last three in the form of ``ops.resample_tables`` (numpy here: host integer and fp64 arithmetic only).

        t   = min(tile, 16 (L // 16))                                      the tile's side: the model's size, or all the axis has
        k   = 1 if L == t else 1 + ceil((L - t) / (t - ov))                ov = min(overlap, t // 2)
        o_i = (2 i (L - t) + (k - 1)) // (2 (k - 1))                       the even spread of k tiles over [0, L - t], rounded half up

    so o_0 = 0, o_{k-1} = L - t, the origins increase strictly and neighbours share at least ``ov`` pixels (= ``overlap`` whenever the axis
    holds a whole tile; on a shorter axis, where t < tile, the overlap is capped at half of the tile that fits).  The weights are
    ``tile_axis_weights`` rounded to fp32 once.  count <= AFX_TILE_MAX_TAPS = 4 by construction (for k >= 3 the real stride exceeds t / 4
    and the rounded origins keep o_{i+4} - o_i >= t); asserted.  Refused with a ValueError naming the argument: L < 16, tile < 32 or no
    multiple of 16, overlap no integer in [0, tile // 2]."""
    for name, v in (('L', L), ('tile', tile), ('overlap', overlap)):
        if isinstance(v, bool) or not isinstance(v, (int, np.integer)):
            raise ValueError(f'{name}: need an integer, got {v!r}')
    L, tile, overlap = int(L), int(tile), int(overlap)
    if L < 16:
        raise ValueError(f'L: an axis of at least 16 pixels, got {L}')
    if tile < 32 or tile % 16:
        raise ValueError(f'tile: a multiple of 16 that is >= 32, got {tile}')
    if not 0 <= overlap <= tile // 2:
        raise ValueError(f'overlap: an integer in [0, tile // 2 = {tile // 2}], got {overlap}')
    t = min(tile, 16 * (L // 16))
    ov = min(overlap, t // 2)
    k = 1 if L == t else 1 + -(-(L - t) // (t - ov))
    origins = np.array([0] if k == 1 else [(2 * i * (L - t) + (k - 1)) // (2 * (k - 1)) for i in range(k)], dtype=np.int32)
    start, count, w = tile_axis_weights(L, t, origins)
    assert origins[0] == 0 and origins[-1] == L - t and (np.diff(origins) > 0).all() and (np.diff(origins) <= t - ov).all()
    assert 1 <= int(count.min()) and int(count.max()) <= AFX_TILE_MAX_TAPS, (L, tile, overlap, int(count.max()))
    return t, origins, start, count, w.astype(np.float32)


class TilePlan(NamedTuple):
    """``tile_plan``'s result: tile iy * kx + ix of side th x tw has its corner at (oy[iy], ox[ix]); y and x are the axes' (start, count, w)."""
    H: int
    W: int
    tile: int
    overlap: int
    th: int
    tw: int
    oy: np.ndarray
    ox: np.ndarray
    y: Tuple[np.ndarray, np.ndarray, np.ndarray]
    x: Tuple[np.ndarray, np.ndarray, np.ndarray]

    @property
    def ky(self) -> int:
        return int(self.oy.size)

    @property
    def kx(self) -> int:
        return int(self.ox.size)

    @property
    def T(self) -> int:
        return self.ky * self.kx


def tile_plan(H: int, W: int, tile: int, overlap: int) -> TilePlan:
    """``tile_axis`` of both axes of an ``H`` x ``W`` canvas: ky x kx tiles of th x tw pixels, tile index iy * kx + ix."""
    try:
        th, oy, *ytab = tile_axis(H, tile, overlap)
        tw, ox, *xtab = tile_axis(W, tile, overlap)
    except ValueError as e:
        if str(e).startswith('L:'):
            raise ValueError(f'H, W: both sides of the canvas must be at least 16 pixels, got {H} x {W}') from None
        raise
    return TilePlan(int(H), int(W), int(tile), int(overlap), th, tw, oy, ox, tuple(ytab), tuple(xtab))


class OutpaintPlan(NamedTuple):
    """``outpaint_plan``'s result: the canvas ``Hc`` x ``Wc``, the photo's rectangle (x0, y0, x1, y1) on it, and the windows (x0, y0, x1, y1),
    all of ``wh`` x ``ww`` pixels, in the order in which they are painted."""
    Hc: int
    Wc: int
    photo: Tuple[int, int, int, int]
    wh: int
    ww: int
    windows: Tuple[Tuple[int, int, int, int], ...]


def _ramp_positive(n: int, lo_inner: bool, hi_inner: bool, blend: int) -> np.ndarray:
    """Along one axis of a rectangle of ``n`` pixels: where the distance to the nearest counted side (``lo_inner`` / ``hi_inner``: the low /
    high side counts) is below ``blend``, which is where max(0, 1 - (d + 1) / (blend + 1)) is > 0, in fp32 as in fp64."""
    i = np.arange(n)
    pos = np.zeros(n, dtype=bool)
    if lo_inner:
        pos |= i < blend
    if hi_inner:
        pos |= (n - 1 - i) < blend
    return pos


def _growth_positions(first: int, side: int, overlap: int, limit: int, forward: bool) -> List[int]:
    """Window origins along the axis a band grows on (``limit`` canvas pixels): the window at ``first`` shifted into the canvas, then every
    further one ``overlap`` pixels before the end of the one before (``forward``: towards ``limit``; else towards 0), until the border."""
    out = [min(max(first, 0), limit - side)]
    while (out[-1] + side < limit) if forward else (out[-1] > 0):
        nxt = out[-1] + side - overlap if forward else out[-1] - side + overlap
        out.append(min(max(nxt, 0), limit - side))
    return out


def _band_positions(a: int, L: int, side: int, overlap: int, limit: int) -> List[int]:
    """Window origins along a band's span [a, a + L): one centred window where the span fits one, else n = ceil((L - side) / (side - overlap))
    + 1 windows spread evenly from a to a + L - side; each shifted into the canvas of ``limit`` pixels."""
    if L <= side:
        starts = [a + (L - side) // 2]
    else:
        n = -(-(L - side) // (side - overlap)) + 1
        starts = [a + (j * (L - side)) // (n - 1) for j in range(n)]
    return [min(max(s, 0), limit - side) for s in starts]


def outpaint_plan(H: int, W: int, left: int, top: int, right: int, bottom: int, tile: int = 1024, overlap: int = 256,
                  blend: int = 32) -> OutpaintPlan:
    """The windows in which ``pipe.outpaint`` extends an ``H`` x ``W`` photo by ``left``, ``top``, ``right``, ``bottom`` pixels: host integer
    arithmetic only.  The canvas is Hc = H + top + bottom by Wc = W + left + right; every window is wh = min(tile, 16 (Hc // 16)) by
    ww = min(tile, 16 (Wc // 16)) pixels.

    The bands go left, right, top, bottom (those with an extent > 0).  The left and right bands span the photo's rows [top, top + H); the
    top and bottom bands span the whole canvas width, the side bands being known by then, so they also paint the corners.  Along the axis
    a band grows on, the first window reaches ``overlap`` pixels back into what is known, each further one starts ``overlap`` pixels before
    the end of the one before, until the canvas border is reached; along the band, a span [a, a + L) that fits one window gets one, centred,
    a longer one n = ceil((L - side) / (side - overlap)) + 1 windows at a + floor(j (L - side) / (n - 1)).  A window that would cross the
    canvas border is shifted inside.  For each growth position come all positions along the band.

    The planner replays the mask state on the host -- ``ops.canvas_extend``'s mask, then the minimum with each window's ramp
    (``ops.canvas_mark``), of both only whether a pixel is > 0, which is exactly ``d < blend`` -- and drops a window that holds no pixel > 0
    when its turn comes.

    Refused with a ValueError: sizes or extents that are not integers, H or W < 1, a negative extent or extents that are all 0, a ``tile``
    that is no multiple of 16 or below 32, a canvas with a side under 16, ``overlap`` outside [1, tile // 2] or not below min(wh, ww),
    ``blend`` outside [0, overlap // 2]."""
    vals = dict(H=H, W=W, left=left, top=top, right=right, bottom=bottom, tile=tile, overlap=overlap, blend=blend)
    for name, v in vals.items():
        if isinstance(v, bool) or not isinstance(v, (int, np.integer)):
            raise ValueError(f'{name}: need an integer, got {v!r}')
    H, W, left, top, right, bottom, tile, overlap, blend = (int(v) for v in vals.values())
    if H < 1 or W < 1:
        raise ValueError(f'H, W: a photo of at least 1 x 1 pixels, got {H} x {W}')
    if min(left, top, right, bottom) < 0 or not (left or top or right or bottom):
        raise ValueError(f'left, top, right, bottom: extents >= 0 with at least one > 0, got {(left, top, right, bottom)}')
    if tile < 32 or tile % 16:
        raise ValueError(f'tile: a multiple of 16 that is >= 32, got {tile}')
    Hc, Wc = H + top + bottom, W + left + right
    if min(Hc, Wc) < 16:
        raise ValueError(f'the canvas is {Hc} x {Wc}: both sides must be at least 16 pixels')
    wh, ww = min(tile, 16 * (Hc // 16)), min(tile, 16 * (Wc // 16))
    if not 1 <= overlap <= tile // 2 or overlap >= min(wh, ww):
        raise ValueError(f'overlap: an integer in [1, tile // 2 = {tile // 2}] below the window\'s sides {wh} x {ww}, got {overlap}')
    if not 0 <= blend <= overlap // 2:
        raise ValueError(f'blend: an integer in [0, overlap // 2 = {overlap // 2}], got {blend}')

    windows: List[Tuple[int, int, int, int]] = []
    if left:
        rows = _band_positions(top, H, wh, overlap, Hc)
        windows += [(x, y, x + ww, y + wh) for x in _growth_positions(left + overlap - ww, ww, overlap, Wc, False) for y in rows]
    if right:
        rows = _band_positions(top, H, wh, overlap, Hc)
        windows += [(x, y, x + ww, y + wh) for x in _growth_positions(left + W - overlap, ww, overlap, Wc, True) for y in rows]
    if top:
        cols = _band_positions(0, Wc, ww, overlap, Wc)
        windows += [(x, y, x + ww, y + wh) for y in _growth_positions(top + overlap - wh, wh, overlap, Hc, False) for x in cols]
    if bottom:
        cols = _band_positions(0, Wc, ww, overlap, Wc)
        windows += [(x, y, x + ww, y + wh) for y in _growth_positions(top + H - overlap, wh, overlap, Hc, True) for x in cols]

    # the replay of the mask state, as booleans: > 0 outside the photo and less than `blend` pixels inside each of its extended sides
    live = np.ones((Hc, Wc), dtype=bool)
    live[top:top + H, left:left + W] = _ramp_positive(H, top > 0, bottom > 0, blend)[:, None] | _ramp_positive(W, left > 0, right > 0, blend)[None, :]
    kept = []
    for x0, y0, x1, y1 in windows:
        view = live[y0:y1, x0:x1]
        if not view.any():
            continue
        view &= _ramp_positive(wh, y0 > 0, y1 < Hc, blend)[:, None] | _ramp_positive(ww, x0 > 0, x1 < Wc, blend)[None, :]
        kept.append((x0, y0, x1, y1))
    return OutpaintPlan(Hc, Wc, (left, top, left + W, top + H), wh, ww, tuple(kept))


def student_sigmas(num_inference_steps: int, total_substeps: int = 128, timestep_ratio: float = 1.0, shift: float = 3.2,
                   num_train_timesteps: int = 1000) -> List[float]:
    """sigma at the start of every student step plus the terminal 0, as the pipelines' ``__call__`` walks them: the raw sub-step grid
    (retrieve_raw_timesteps) through the static shift of FlowMatchEulerDiscreteScheduler in fp32, every step reading the first
    sub-step of its segment as ``timestep / num_train_timesteps``.  For samplers outside the pipelines (ArcFlowDistiller.sample_student)."""
    raw, per_step, total = retrieve_raw_timesteps(num_inference_steps, total_substeps, timestep_ratio)
    sch = FlowMatchEulerDiscreteScheduler(num_train_timesteps=num_train_timesteps, shift=shift, use_dynamic_shifting=False)
    ts = sch.set_timesteps(sigmas=raw).float().tolist()
    out, tid = [], 0
    for n in per_step:
        out.append(ts[tid] / num_train_timesteps)
        tid += n
    assert tid == total == len(ts)
    return out + [0.0]


def student_edit_sigmas(num_inference_steps: int, total_substeps: int = 128, timestep_ratio: float = 1.0, shift: float = 3.2,
                        strength: float = 1.0, num_train_timesteps: int = 1000) -> List[float]:
    """``student_sigmas`` of an edit, as the pipelines' ``_denoise`` walks them: the raw grid of ``edit_raw_timesteps`` (every raw time
    multiplied by ``strength`` in (0, 1]) through the same static shift in fp32, every step reading the first sub-step of its segment, plus
    the terminal 0.  The first entry is the sigma the source is noised to.  strength == 1.0 returns ``student_sigmas``' list."""
    raw, per_step, total = edit_raw_timesteps(num_inference_steps, total_substeps, timestep_ratio, strength)
    sch = FlowMatchEulerDiscreteScheduler(num_train_timesteps=num_train_timesteps, shift=shift, use_dynamic_shifting=False)
    ts = sch.set_timesteps(sigmas=raw).float().tolist()
    out, tid = [], 0
    for n in per_step:
        out.append(ts[tid] / num_train_timesteps)
        tid += n
    assert tid == total == len(ts)
    return out + [0.0]


class _Config(dict):
    """dict with attribute access, like diffusers' FrozenDict configs."""
    __getattr__ = dict.get

    def get(self, k, default=None):          # noqa: D401 - keep dict.get semantics
        return super().get(k, default)


class FlowMatchEulerDiscreteScheduler:
    """The subset of diffusers' scheduler the ArcFlow pipelines touch: config, from_config(),
    set_begin_index(), set_timesteps(sigmas=..., mu=...), .timesteps / .sigmas.

    sigma' = shift * s / (1 + (shift-1) s) for the static shift; with use_dynamic_shifting the
    exponential time shift exp(mu) / (exp(mu) + (1/s - 1)) of the stock FLUX pipeline.
    """
    _DEFAULTS = dict(num_train_timesteps=1000, shift=1.0, use_dynamic_shifting=False, base_shift=0.5,
                     max_shift=1.15, base_image_seq_len=256, max_image_seq_len=4096, shift_terminal=None)

    def __init__(self, **kwargs: Any):
        cfg = dict(self._DEFAULTS)
        cfg.update(kwargs)
        self.config = _Config(cfg)
        self.timesteps: Optional[torch.Tensor] = None
        self.sigmas: Optional[torch.Tensor] = None
        self._begin_index = None

    @classmethod
    def from_config(cls, config: Optional[Dict[str, Any]] = None, **overrides: Any):
        cfg = dict(config or {})
        cfg.update(overrides)
        cfg = {k: v for k, v in cfg.items() if not k.startswith('_')}
        return cls(**cfg)

    def set_begin_index(self, begin_index: int = 0):
        self._begin_index = begin_index

    def set_timesteps(self, num_inference_steps: Optional[int] = None, device=None,
                      sigmas: Optional[List[float]] = None, mu: Optional[float] = None):
        if sigmas is None:
            n = num_inference_steps
            sigmas = np.linspace(1.0, 1.0 / self.config.num_train_timesteps, n)
        s = np.asarray(sigmas, dtype=np.float32)
        if self.config.use_dynamic_shifting:
            if mu is None:
                raise ValueError('mu is required with use_dynamic_shifting')
            s = (math.exp(mu) / (math.exp(mu) + (1.0 / s - 1.0))).astype(np.float32)
        else:
            sh = np.float32(self.config.shift)
            s = (sh * s / (np.float32(1) + (sh - np.float32(1)) * s)).astype(np.float32)
        if self.config.shift_terminal:
            one_minus = 1 - s
            s = (1 - one_minus / (one_minus[-1] / (1 - self.config.shift_terminal))).astype(np.float32)
        sig = torch.from_numpy(s)
        self.timesteps = (sig * self.config.num_train_timesteps).to(device)
        self.sigmas = torch.cat([sig, torch.zeros(1)]).to(device)
        return self.timesteps


def calculate_shift(image_seq_len, base_seq_len=256, max_seq_len=4096, base_shift=0.5, max_shift=1.15):
    m = (max_shift - base_shift) / (max_seq_len - base_seq_len)
    return image_seq_len * m + (base_shift - m * base_seq_len)


class _FlowSchedulerTables:
    """What the reference's own flow schedulers share (schedulers/flow_euler_ode.py:20-118 and schedulers/flow_sde.py:21-111 are the
    same text up to ``step()``): ``config``, ``from_config()``, ``get_shift()``, ``stretch_to_terminal()``, ``set_timesteps(n, seq_len=...)``
    and the step index.  A subclass sets ``_DEFAULTS`` and adds ``step()``.

    Grid: n points of linspace(1, 0, endpoint=False), warped by sigma' = s sigma / (1 + (s - 1) sigma) with the static ``shift`` or,
    with ``use_dynamic_shifting``, s = exp(logshift) interpolated linearly in ``seq_len`` between (base_seq_len, base_logshift)
    and (max_seq_len, max_logshift); optionally stretched so that the last sigma is ``terminal_sigma``; a trailing 0 is appended to
    ``sigmas`` (the last step lands on the clean sample)."""
    order = 1
    _DEFAULTS: Dict[str, Any] = {}

    def __init__(self, num_train_timesteps: int = 1000, **kwargs: Any):
        cfg = dict(self._DEFAULTS)
        cfg['num_train_timesteps'] = num_train_timesteps
        unknown = set(kwargs) - set(cfg)
        if unknown:
            raise TypeError(f'{type(self).__name__} got unexpected arguments {sorted(unknown)}')
        cfg.update(kwargs)
        self.config = _Config(cfg)
        shift = self.config.shift
        sigmas = torch.from_numpy(1 - np.linspace(0, 1, num_train_timesteps, dtype=np.float32, endpoint=False))
        self.sigmas = shift * sigmas / (1 + (shift - 1) * sigmas)
        self.timesteps = self.sigmas * num_train_timesteps
        self._step_index = None
        self._begin_index = None
        self.sigma_min = self.sigmas[-1].item()
        self.sigma_max = self.sigmas[0].item()

    @classmethod
    def from_config(cls, config: Optional[Dict[str, Any]] = None, **overrides: Any):
        cfg = dict(config or {})
        cfg.update(overrides)
        cfg = {k: v for k, v in cfg.items() if k in cls._DEFAULTS}       # a foreign scheduler's config: only the shared keys apply
        return cls(**cfg)

    @property
    def step_index(self):
        return self._step_index

    @property
    def begin_index(self):
        return self._begin_index

    def set_begin_index(self, begin_index: int = 0):
        self._begin_index = begin_index

    def get_shift(self, seq_len=None):
        c = self.config
        if c.use_dynamic_shifting and seq_len is not None:
            m = (c.max_logshift - c.base_logshift) / (c.max_seq_len - c.base_seq_len)
            logshift = (seq_len - c.base_seq_len) * m + c.base_logshift
            return torch.exp(logshift) if isinstance(logshift, torch.Tensor) else np.exp(logshift)
        return c.shift

    def stretch_to_terminal(self, sigma: torch.Tensor) -> torch.Tensor:
        one_minus_sigma = 1 - sigma
        return 1 - (one_minus_sigma * (1 - self.config.terminal_sigma) / one_minus_sigma[-1])

    def set_timesteps(self, num_inference_steps: int, seq_len=None, device=None):
        self.num_inference_steps = num_inference_steps
        sigmas = torch.from_numpy(np.linspace(1, 0, num_inference_steps, dtype=np.float32, endpoint=False))
        shift = self.get_shift(seq_len=seq_len)
        sigmas = shift * sigmas / (1 + (shift - 1) * sigmas)
        if self.config.terminal_sigma is not None:
            sigmas = self.stretch_to_terminal(sigmas)
        self.timesteps = (sigmas * self.config.num_train_timesteps).to(device)
        self.sigmas = torch.cat([sigmas, torch.zeros(1)])
        self._step_index = None
        self._begin_index = None
        return self.timesteps

    def index_for_timestep(self, timestep, schedule_timesteps=None):
        ts = self.timesteps if schedule_timesteps is None else schedule_timesteps
        indices = (ts == timestep).nonzero()
        return indices[1 if len(indices) > 1 else 0].item()

    def _begin_step(self, timestep, prediction_type: str) -> int:
        """The checks both ``step()``s open with; -> the index of the step about to be taken."""
        if prediction_type != 'u':
            raise NotImplementedError(f"{type(self).__name__}.step: only prediction_type='u' (the teacher predicts a velocity)")
        if isinstance(timestep, int) or (isinstance(timestep, torch.Tensor) and not timestep.is_floating_point()):
            raise ValueError('pass one of scheduler.timesteps as the timestep, not an integer index')
        if self._step_index is None:
            if self._begin_index is None:
                t = timestep.to(self.timesteps.device) if isinstance(timestep, torch.Tensor) else timestep
                self._step_index = self.index_for_timestep(t)
            else:
                self._step_index = self._begin_index
        return self._step_index

    def __len__(self):
        return self.config.num_train_timesteps


class FlowEulerODEScheduler(_FlowSchedulerTables):
    """The reference's own Euler ODE scheduler (lakonlab/models/diffusions/schedulers/flow_euler_ode.py:20-164), the default
    ``sampler`` of ``GaussianFlow.forward_test``, without diffusers: ``config``, ``from_config()``, ``get_shift()``,
    ``stretch_to_terminal()``, ``set_timesteps(n, seq_len=...)`` and ``step()`` for ``prediction_type='u'``.  Same fp32 operations in the
    same order as the reference (tests/golden/g12_teacher_sampler.npz)."""
    _DEFAULTS = dict(num_train_timesteps=1000, shift=1.0, use_dynamic_shifting=False, base_seq_len=256, max_seq_len=4096,
                     base_logshift=0.5, max_logshift=1.15, terminal_sigma=None)

    def step(self, model_output: torch.Tensor, timestep, sample: torch.Tensor, generator=None, return_dict: bool = True,
             prediction_type: str = 'u'):
        """prev_sample = sample + model_output (sigma_next - sigma) in fp32, cast back to model_output's dtype."""
        i = self._begin_step(timestep, prediction_type)
        ori_dtype = model_output.dtype
        sigma = self.sigmas[i]
        sigma_to = self.sigmas[i + 1]
        dt = (sigma_to - sigma).to(sample.device)
        prev_sample = (sample.to(torch.float32) + model_output.to(torch.float32) * dt).to(ori_dtype)
        self._step_index += 1
        if not return_dict:
            return (prev_sample,)
        return _Config(prev_sample=prev_sample)


class FlowSDEScheduler(_FlowSchedulerTables):
    """The reference's stochastic scheduler (lakonlab/models/diffusions/schedulers/flow_sde.py:21-180; ``sampler='FlowSDE'`` in a
    ``test_cfg``) without diffusers: the tables of FlowEulerODEScheduler, and a ``step()`` that re-injects fresh noise with a strength
    set by ``h`` -- a float, or the string ``'inf'``.  With x0 = x - sigma u and eps = x + (1 - sigma) u the predictions of the clean
    sample and of the noise,

        prev = (1 - sigma_to) x0 + sigma_to (m eps + sqrt(max(1 - m^2, 0)) z),      z ~ N(0, 1) fresh per step,
        m = (sigma_to (1 - sigma) / max(sigma (1 - sigma_to), 1e-6)) ^ (h^2)

    h = 0 gives m = 1: the ODE step (algebraically x + u (sigma_to - sigma)); h = 'inf' gives m = 0: the predicted clean sample is
    re-noised completely.  Same fp32 operations in the same order as the reference (tests/golden/g13_sde_sampler.npz)."""
    _DEFAULTS = dict(FlowEulerODEScheduler._DEFAULTS, h=1.0)

    def __init__(self, num_train_timesteps: int = 1000, **kwargs: Any):
        super().__init__(num_train_timesteps, **kwargs)
        h = self.config.h
        if isinstance(h, str) and h != 'inf':
            raise ValueError(f"h: a float or the string 'inf', got {h!r}")

    def coefficients(self, i: int) -> Tuple[torch.Tensor, torch.Tensor, torch.Tensor, torch.Tensor]:
        """-> (sigma, sigma_to, m, c_noise) of step i as fp32 scalars, c_noise = sqrt(max(1 - m^2, 0)): what ``step()`` mixes with,
        and what the fused step kernel (afx_teacher_sde_step) is handed.  Needs ``set_timesteps()``."""
        sigma, sigma_to = self.sigmas[i], self.sigmas[i + 1]
        alpha, alpha_to = 1 - sigma, 1 - sigma_to
        h = self.config.h
        if h == 'inf':
            m = torch.zeros_like(sigma)
        elif h == 0.0:
            m = torch.ones_like(sigma)
        else:
            if not h > 0.0:
                raise ValueError(f'h must be >= 0 (or the string \'inf\'), got {h!r}')
            m = (sigma_to * alpha / (sigma * alpha_to).clamp(min=1e-6)) ** (h * h)
        return sigma, sigma_to, m, (1 - m.square()).clamp(min=0).sqrt()

    def step(self, model_output: torch.Tensor, timestep, sample: torch.Tensor, generator=None, return_dict: bool = True,
             prediction_type: str = 'u', noise: Optional[torch.Tensor] = None):
        """One stochastic step in fp32, cast back to model_output's dtype.  noise: the step's N(0, 1) draw (default: torch.randn of
        model_output's shape on its device from ``generator``)."""
        i = self._begin_step(timestep, prediction_type)
        ori_dtype = model_output.dtype
        sample = sample.to(torch.float32)
        model_output = model_output.to(torch.float32)
        sigma, sigma_to, m, c_noise = self.coefficients(i)
        alpha, alpha_to = 1 - sigma, 1 - sigma_to
        x0 = sample - sigma * model_output
        epsilon = sample + alpha * model_output
        if noise is None:
            noise = torch.randn(model_output.shape, generator=generator, device=model_output.device, dtype=torch.float32)
        prev_sample = (alpha_to * x0 + sigma_to * (m * epsilon + c_noise * noise)).to(ori_dtype)
        self._step_index += 1
        if not return_dict:
            return (prev_sample,)
        return _Config(prev_sample=prev_sample)


class UniPCStep(NamedTuple):
    """The scalars of one UniPC step (FlowUniPCScheduler.coefficients), fp64: with m_t = x - sigma u,
        x_c    = corrector . (last_sample, m_t, m[-1], m[-2], m[-3])          (corrector None: x_c = x, the first step of a roll)
        x_next = predictor . (x_c, m_t, m[-1], m[-2])
    m[-k] the x0-prediction of k steps ago.  A history term beyond the step's order has weight 0.0 and is not read."""
    sigma: float
    corrector: Optional[Tuple[float, float, float, float, float]]
    predictor: Tuple[float, float, float, float]
    corrector_order: int
    predictor_order: int

    def row(self) -> List[float]:
        """The ten values afx_teacher_unipc_step takes per sample: sigma, the corrector's five (zeros without one), the predictor's four."""
        return [self.sigma, *(self.corrector or (0.0,) * 5), *self.predictor]


class FlowUniPCScheduler(_FlowSchedulerTables):
    """The reference's adapter scheduler (lakonlab/models/diffusions/schedulers/flow_adapter.py, ``sampler='FlowAdapter'`` in a ``test_cfg``)
    on its default ``base_scheduler='UniPCMultistep'``, without diffusers: the tables of FlowEulerODEScheduler, ``base_sigmas`` =
    ``sigmas.clamp(max=1 - eps)`` for the solver (flow_adapter.py:148), and UniPC (predictor + corrector, x0-prediction, flow sigmas,
    ``lower_order_final``, final sigma 0) of order ``solver_order`` in {1, 2, 3} with ``solver_type`` 'bh1' / 'bh2'.

    The multistep arithmetic is diffusers' ``UniPCMultistepScheduler`` AS RECALLED (DESIGN.md 6.1 "Multistep sampling" writes it out): no
    fixture pins it -- parity unpinned.  With s the clamped sigmas, alpha = 1 - s, lambda = log alpha - log s, step i does
    m_t = x - s_i u; for i past the first step of the roll the corrector re-evaluates x with m_t; then the predictor advances to s_{i+1}.
    Both are linear in (last_sample | x, m_t, past m's): ``coefficients(i)`` evaluates their weights in fp64 on the host, which is what
    ``step()`` applies in torch and the fused kernel (afx_teacher_unipc_step) per element."""
    _DEFAULTS = dict(FlowEulerODEScheduler._DEFAULTS, solver_order=2, solver_type='bh2', eps=1e-4)

    def __init__(self, num_train_timesteps: int = 1000, **kwargs: Any):
        super().__init__(num_train_timesteps, **kwargs)
        c = self.config
        if isinstance(c.solver_order, bool) or c.solver_order not in (1, 2, 3):
            raise ValueError(f'solver_order: one of 1, 2, 3, got {c.solver_order!r}')
        if c.solver_type not in ('bh1', 'bh2'):
            raise ValueError(f"solver_type: 'bh1' or 'bh2', got {c.solver_type!r}")
        if not 0.0 < float(c.eps) < 1.0:
            raise ValueError(f'eps must lie in (0, 1), got {c.eps!r}')
        self.base_sigmas = self.sigmas.clamp(max=1 - c.eps)
        self._reset()

    def _reset(self):
        self.model_outputs: List[torch.Tensor] = []          # past x0-predictions, oldest first, at most solver_order of them
        self.last_sample: Optional[torch.Tensor] = None
        self.lower_order_nums = 0
        self.this_order: Optional[int] = None
        self._first_index: Optional[int] = None              # the step the current roll began with

    def set_timesteps(self, num_inference_steps: int, seq_len=None, device=None):
        ts = super().set_timesteps(num_inference_steps, seq_len=seq_len, device=device)
        self.base_sigmas = self.sigmas.clamp(max=1 - self.config.eps)
        self._reset()
        return ts

    def orders(self, i: int, begin: int = 0) -> Tuple[int, int]:
        """-> (corrector order, predictor order) of step i in a roll that began at step ``begin`` with an empty history; corrector order 0
        = no corrector (i == begin).  The predictor's is diffusers' ``this_order`` = min(solver_order, n - i, lower_order_nums + 1) with
        lower_order_nums = min(i - begin, solver_order); the corrector's is the previous step's ``this_order``."""
        n, so, j = self.num_inference_steps, self.config.solver_order, i - begin
        if not 0 <= begin <= i < n:
            raise ValueError(f'step {i} of a roll from step {begin} of {n}')
        return (min(so, n - i + 1, j) if j > 0 else 0), min(so, n - i, min(j, so) + 1)

    def _rho(self, order: int, rks: List[float], hh: float, predictor: bool) -> Tuple[List[float], float, float]:
        """-> (rho over rks, h phi_1, B) of one UniPC update with hh = -h, finite.  rks = [r_1 .. r_{order-1}, 1]."""
        h_phi_1 = math.expm1(hh)
        B = h_phi_1 if self.config.solver_type == 'bh2' else hh
        phi, f, b = h_phi_1 / hh - 1.0, 1.0, []
        for j in range(1, order + 1):
            b.append(phi * f / B)
            f *= j + 1
            phi = phi / hh - 1.0 / f
        R = [[r ** j for r in rks] for j in range(order)]
        if predictor:                                       # the last column (r = 1, the point not yet evaluated) is the corrector's
            if order == 1:
                rho: List[float] = []
            elif order == 2:
                rho = [0.5]
            else:
                rho = np.linalg.solve(np.array(R, dtype=np.float64)[:-1, :-1], np.array(b[:-1], dtype=np.float64)).tolist()
        else:
            rho = [0.5] if order == 1 else np.linalg.solve(np.array(R, dtype=np.float64), np.array(b, dtype=np.float64)).tolist()
        return rho, h_phi_1, B

    def coefficients(self, i: int, begin: Optional[int] = None) -> UniPCStep:
        """The flattened scalars of step i, in fp64 from the fp32 table ``base_sigmas``; ``begin``: the first step of the roll (default: the
        one ``step()`` began with, else 0), where the history is empty.  Needs ``set_timesteps()``.

        Flattening: each D_k = (m[-(k+1)] - m0) / r_k puts rho_k / r_k on m[-(k+1)] and takes the same from m0, so with
        a = alpha(s_to), g_k = rho_k / r_k:
          corrector (s_to = s_i, m0 = m[-1]):  last_sample: s_i / s_{i-1};  m_t: -a B rho_last;  m[-(k+1)]: -a B g_k;
                                               m[-1]: -a h phi_1 + a B (sum_k g_k + rho_last)
          predictor (s_to = s_{i+1}, m0 = m_t): x_c: s_{i+1} / s_i;  m[-k]: -a B g_k;  m_t: -a h phi_1 + a B sum_k g_k
        The step landing on sigma 0 has h = +inf: order 1 (lower_order_final), expm1(-inf) = -1, so x_next = 0 x_c + 1 m_t exactly."""
        if begin is None:
            begin = self._first_index if self._first_index is not None else 0
        oc, op = self.orders(i, begin)
        s = [float(v) for v in self.base_sigmas.double().tolist()]
        lam = [math.log1p(-v) - math.log(v) if v > 0.0 else math.inf for v in s]

        def ratios(order: int, base: int, h: float) -> List[float]:
            return [(lam[base - k] - lam[base]) / h for k in range(1, order)] + [1.0]

        corrector = None
        if oc:
            h = lam[i] - lam[i - 1]
            if not (h > 0.0 and math.isfinite(h)):
                raise ValueError(f'UniPC needs strictly decreasing sigmas in (0, 1): sigma[{i - 1}] = {s[i - 1]}, sigma[{i}] = {s[i]} (after the clamp to 1 - eps)')
            rks = ratios(oc, i - 1, h)
            rho, h_phi_1, B = self._rho(oc, rks, -h, predictor=False)
            a = 1.0 - s[i]
            g = [rho[k] / rks[k] for k in range(oc - 1)]
            w = [s[i] / s[i - 1], -a * B * rho[-1], -a * h_phi_1 + a * B * (sum(g) + rho[-1])] + [-a * B * gk for gk in g]
            corrector = tuple(w + [0.0] * (5 - len(w)))
        if s[i + 1] == 0.0:
            if op != 1:
                raise ValueError('a step onto sigma 0 that is not the last step of the schedule')
            predictor = (0.0, 1.0, 0.0, 0.0)
        else:
            h = lam[i + 1] - lam[i]
            if not (h > 0.0 and math.isfinite(h)):
                raise ValueError(f'UniPC needs strictly decreasing sigmas in (0, 1): sigma[{i}] = {s[i]}, sigma[{i + 1}] = {s[i + 1]} (after the clamp to 1 - eps)')
            rks = ratios(op, i, h)
            rho, h_phi_1, B = self._rho(op, rks, -h, predictor=True)
            a = 1.0 - s[i + 1]
            g = [rho[k] / rks[k] for k in range(op - 1)]
            w = [s[i + 1] / s[i], -a * h_phi_1 + a * B * sum(g)] + [-a * B * gk for gk in g]
            predictor = tuple(w + [0.0] * (4 - len(w)))
        return UniPCStep(s[i], corrector, predictor, oc, op)

    def step(self, model_output: torch.Tensor, timestep, sample: torch.Tensor, generator=None, return_dict: bool = True,
             prediction_type: str = 'u'):
        """One UniPC step in fp32 with the weights of ``coefficients()`` rounded to fp32, cast back to model_output's dtype.  The first
        ``step()`` after ``set_timesteps()`` begins a roll: an empty history, at ``begin_index`` or at ``timestep``'s index."""
        i = self._begin_step(timestep, prediction_type)
        if self._first_index is None:
            self._first_index = i
        ori_dtype = model_output.dtype
        x = sample.to(torch.float32)
        u = model_output.to(torch.float32)
        co = self.coefficients(i)
        m_t = x - torch.tensor(co.sigma, dtype=torch.float32) * u
        hist = self.model_outputs[::-1]                                  # hist[k - 1] = m[-k]
        f32 = lambda v: torch.tensor(v, dtype=torch.float32)             # noqa: E731
        if co.corrector is not None:
            cl, cm, *ch = co.corrector
            x_c = f32(cl) * self.last_sample
            for k in range(co.corrector_order):
                x_c = x_c + f32(ch[k]) * hist[k]
            x_c = x_c + f32(cm) * m_t
        else:
            x_c = x
        px, pm, *ph = co.predictor
        prev = f32(px) * x_c
        for k in range(co.predictor_order - 1):
            prev = prev + f32(ph[k]) * hist[k]
        prev_sample = (prev + f32(pm) * m_t).to(ori_dtype)
        self.model_outputs = (self.model_outputs + [m_t])[-self.config.solver_order:]
        self.last_sample = x_c
        self.this_order = co.predictor_order
        if self.lower_order_nums < self.config.solver_order:
            self.lower_order_nums += 1
        self._step_index += 1
        if not return_dict:
            return (prev_sample,)
        return _Config(prev_sample=prev_sample)
