"""afx_canvas_extend and afx_canvas_mark per element against the numpy restatement of tests/outpaint_ref.py.  The canvas is a bit copy and is
held by equality.  The mask is ramp(d) = 1.0f - float(d + 1) / float(blend + 1) in fp32: the quotient rounds once and so does the
subtraction, both results lie in [0, 1], so each error is at most 2^-24 and the bound against fp64 is 2^-23; where it is > 0, and its exact
1 and 0 values, are held by equality.  The shapes are the smallest at which the indexing can go wrong: a pad larger than the mirror's
period, an unextended side, an odd row pitch, a one-row photo, a batch of two, a blend wider than the photo.  On the parent commit every test
here fails: ``ops.canvas_extend`` and ``ops.canvas_mark`` do not exist."""
import numpy as np
import pytest
import torch

import outpaint_ref as R

pytestmark = pytest.mark.gpu

TOL = 2.0 ** -23
CASES = [((1, 5, 7), (3, 0, 19, 2)),           # a pad larger than 2 (n - 1), an unextended side, an odd row pitch
         ((1, 1, 4), (2, 3, 0, 0)),            # n == 1
         ((2, 40, 56), (16, 24, 8, 0))]        # a batch of two; the chunks of four pixels run over rows and over the first image's end


def _photo(shape, seed):
    return np.random.default_rng(seed).integers(0, 256, shape + (3,), dtype=np.uint8)


def _check_mask(got, want):
    assert got.dtype == np.float32 and got.shape == want.shape
    assert np.abs(got.astype(np.float64) - want).max() <= TOL
    assert np.array_equal(got > 0, want > 0) and np.array_equal(got == 1, want == 1) and np.array_equal(got == 0, want == 0)
    assert got.min() >= 0 and got.max() <= 1


@pytest.mark.parametrize('fill', ['edge', 'reflect'])
@pytest.mark.parametrize('case', range(len(CASES)))
def test_canvas_extend_per_element(case, fill):
    from arcflow_amd import ops
    shape, (left, top, right, bottom) = CASES[case]
    photo = _photo(shape, 7 + case)
    src = torch.from_numpy(photo).cuda()
    for blend in (0, 1, 5, 64):
        canvas, mask = ops.canvas_extend(src, left, top, right, bottom, fill=fill, blend=blend)
        torch.cuda.synchronize()
        B, H, W = shape
        assert canvas.dtype == torch.uint8 and canvas.shape == (B, H + top + bottom, W + left + right, 3)
        assert mask.dtype == torch.float32 and mask.shape == (1, 1, H + top + bottom, W + left + right)
        want_c, want_m = R.canvas_extend(photo, left, top, right, bottom, fill, blend)
        assert np.array_equal(canvas.cpu().numpy(), want_c), (case, fill, blend)
        assert np.array_equal(want_c, np.pad(photo, ((0, 0), (top, bottom), (left, right), (0, 0)), mode=fill))
        assert np.array_equal(canvas[:, top:top + H, left:left + W].cpu().numpy(), photo)          # inside the rectangle the canvas is the photo
        _check_mask(mask[0, 0].cpu().numpy(), want_m)
        if blend == 0:
            inside = mask[0, 0, top:top + H, left:left + W]
            assert (inside == 0).all() and mask.sum().item() == mask.numel() - H * W               # a binary mask
    again_c, again_m = ops.canvas_extend(src, left, top, right, bottom, fill=fill, blend=64)
    assert torch.equal(again_c, canvas) and torch.equal(again_m.view(torch.int32), mask.view(torch.int32))
    assert torch.equal(src.cpu(), torch.from_numpy(photo))                                          # the source is only read


def test_canvas_extend_at_any_alignment_and_inside_its_buffers():
    """A photo one byte into its buffer (the 12-byte loads are at any alignment), a canvas at an odd address (byte stores) and a mask at a
    4-byte address that is no multiple of 16 (single stores), through the C ABI; the bytes and floats around the outputs stay as they were."""
    import ctypes as C
    from arcflow_amd import _lib
    photo = _photo((2, 9, 13), 3)
    left, top, right, bottom, blend = 5, 1, 7, 29, 3          # a 39 x 25 canvas: the last chunk of four pixels is short
    Hc, Wc = 9 + top + bottom, 13 + left + right
    want_c, want_m = R.canvas_extend(photo, left, top, right, bottom, 'reflect', blend)
    sbuf = torch.zeros(photo.size + 1, dtype=torch.uint8, device='cuda')
    sbuf[1:] = torch.from_numpy(photo).cuda().flatten()
    cbuf = torch.full((want_c.size + 16,), 0xAB, dtype=torch.uint8, device='cuda')
    mbuf = torch.full((want_m.size + 8,), -7.0, dtype=torch.float32, device='cuda')
    for c_off, m_off in ((1, 1), (3, 3), (8, 4), (2, 2)):
        cbuf.fill_(0xAB)
        mbuf.fill_(-7.0)
        src, canvas, mask = sbuf.data_ptr() + 1, cbuf.data_ptr() + c_off, mbuf.data_ptr() + 4 * m_off
        _lib.check(_lib.load().afx_canvas_extend(C.c_void_p(src), 2, 9, 13, left, top, right, bottom, _lib.AFX_FILL_REFLECT, blend,
                                                 C.c_void_p(canvas), C.c_void_p(mask), C.c_void_p(torch.cuda.current_stream().cuda_stream)))
        torch.cuda.synchronize()
        got_c, got_m = cbuf.cpu().numpy(), mbuf.cpu().numpy()
        assert np.array_equal(got_c[c_off:c_off + want_c.size].reshape(want_c.shape), want_c), (c_off, m_off)
        assert (got_c[:c_off] == 0xAB).all() and (got_c[c_off + want_c.size:] == 0xAB).all()
        _check_mask(got_m[m_off:m_off + Hc * Wc].reshape(Hc, Wc), want_m)
        assert (got_m[:m_off] == -7.0).all() and (got_m[m_off + Hc * Wc:] == -7.0).all()


WINDOWS = [(16, 8, 48, 40),        # touches no border
           (0, 8, 32, 40),         # the left border
           (48, 16, 80, 48),       # the right and the bottom border
           (0, 0, 80, 48),         # all four: the whole area becomes 0
           (37, 21, 38, 22),       # 1 x 1
           (3, 5, 78, 6)]          # one row, no multiple of four at either end


@pytest.mark.parametrize('shape', [(48, 80), (47, 79)])          # a row pitch of whole 16-byte quads, and one of neither
def test_canvas_mark_per_element(shape):
    from arcflow_amd import ops
    Hc, Wc = shape
    rng = np.random.default_rng(5)
    start = rng.random(shape, dtype=np.float32)
    start[rng.random(shape) < 0.2] = 1.0
    start[rng.random(shape) < 0.2] = 0.0
    for blend in (0, 1, 5, 64):
        for win in WINDOWS:
            x0, y0, x1, y1 = (min(win[0], Wc - 1), min(win[1], Hc - 1), min(win[2], Wc), min(win[3], Hc))
            M = torch.from_numpy(start).cuda()[None, None].contiguous()
            assert ops.canvas_mark(M, (x0, y0, x1, y1), blend) is M
            want = R.canvas_mark(start.astype(np.float64), (x0, y0, x1, y1), blend)
            got = M[0, 0].cpu().numpy()
            _check_mask(got, want)
            outside = np.ones(shape, dtype=bool)
            outside[y0:y1, x0:x1] = False
            assert np.array_equal(got[outside].view(np.int32), start[outside].view(np.int32)), (win, blend)       # nothing outside the window changes
            if (x0, y0, x1, y1) == (0, 0, Wc, Hc):
                assert (got == 0).all()
            # a second, overlapping mark: the state only decreases, and the order does not matter
            second = (8, 4, 40, 36)
            first = M.clone()
            ops.canvas_mark(M, second, blend)
            want2 = R.canvas_mark(want, second, blend)
            _check_mask(M[0, 0].cpu().numpy(), want2)
            assert (M <= first).all()
            other = torch.from_numpy(start).cuda().contiguous()                                                   # the [Hc, Wc] form
            ops.canvas_mark(other, second, blend)
            ops.canvas_mark(other, (x0, y0, x1, y1), blend)
            assert torch.equal(other.view(torch.int32), M[0, 0].view(torch.int32)), (win, blend)


def test_extend_then_marks_replay_the_plan_to_zero():
    """The device state over the windows of a plan ends at 0 everywhere, and is > 0 where the host replay says so on the way."""
    from arcflow_amd import ops, schedule
    H, W, ext, blend = 40, 56, (16, 24, 8, 0), 4
    plan = schedule.outpaint_plan(H, W, *ext, tile=32, overlap=8, blend=blend)
    _, M = ops.canvas_extend(torch.from_numpy(_photo((1, H, W), 1)).cuda(), *ext, fill='edge', blend=blend)
    _, want = R.canvas_extend(np.zeros((1, H, W, 3), dtype=np.uint8), *ext, 'edge', blend)
    for win in plan.windows:
        x0, y0, x1, y1 = win
        assert (M[0, 0, y0:y1, x0:x1] > 0).any()
        ops.canvas_mark(M, win, blend)
        want = R.canvas_mark(want, win, blend)
        assert np.array_equal(M[0, 0].cpu().numpy() > 0, want > 0)
    assert (M == 0).all()
