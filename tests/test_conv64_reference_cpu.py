"""The fp64 convolution reference of tests/test_hip_vae_fp64.py (bf16_parity.conv64: shifted matmuls on the padded NHWC grid) against F.conv2d in fp64 on
the CPU at 1e-12: stride 1, stride 2 with right / bottom padding, nearest-2x followed by the convolution, and the four 2x2 phase convolutions of the
folded upsample scattered to the 2x grid (with fp64 phase weights, so that only the indexing is under test).  Also: the layer table of that file against
the weight shapes of the released models."""
import torch
import torch.nn.functional as F
from bf16_parity import conv64


def _case(seed, H, W, ci, co):
    g = torch.Generator().manual_seed(seed)
    return (torch.randn(H, W, ci, generator=g, dtype=torch.float64), torch.randn(co, ci, 3, 3, generator=g, dtype=torch.float64) * 0.1,
            torch.randn(co, generator=g, dtype=torch.float64))


def _nchw(x):
    return x.permute(2, 0, 1)[None]


def _close(y, ref):
    assert y.shape == ref.shape
    assert (y - ref).abs().max().item() <= 1e-12 * max(1.0, ref.abs().max().item())


def test_conv64_stride1_vs_conv2d():
    x, w, b = _case(0, 7, 10, 5, 6)
    y, mag, fl = conv64(F.pad(x, (0, 0, 1, 1, 1, 1)), w, b, 7, 10)
    _close(y, F.conv2d(_nchw(x), w, b, padding=1)[0].permute(1, 2, 0))
    _close(mag, F.conv2d(_nchw(x.abs()), w.abs(), b.abs(), padding=1)[0].permute(1, 2, 0))
    assert torch.equal(fl, (9 * 5 // 32 + 33) * 2.0 ** -24 * mag)
    # one tap left out = the convolution with that tap's weights zeroed
    w0 = w.clone()
    w0[:, :, 1, 1] = 0
    _close(conv64(F.pad(x, (0, 0, 1, 1, 1, 1)), w, b, 7, 10, skip=(1, 1))[0], F.conv2d(_nchw(x), w0, b, padding=1)[0].permute(1, 2, 0))


def test_conv64_stride2_right_bottom_padding_vs_conv2d():
    x, w, b = _case(1, 8, 12, 4, 3)
    y, _, _ = conv64(F.pad(x, (0, 0, 0, 1, 0, 1)), w, b, 4, 6, stride=2)
    _close(y, F.conv2d(F.pad(_nchw(x), (0, 1, 0, 1)), w, b, stride=2)[0].permute(1, 2, 0))
    # on a grid padded on all four sides (as the kernels' grids are) the same convolution starts at offset (1, 1)
    y1, _, _ = conv64(F.pad(x, (0, 0, 1, 1, 1, 1)), w, b, 4, 6, stride=2, oy=1, ox=1)
    assert torch.equal(y, y1)


def test_conv64_nearest2x_then_conv_and_its_four_phases_vs_conv2d():
    from arcflow_amd.vae import phase_weights
    x, w, b = _case(2, 5, 6, 8, 4)
    up = x.repeat_interleave(2, 0).repeat_interleave(2, 1)
    ref = F.conv2d(F.interpolate(_nchw(x), scale_factor=2, mode='nearest'), w, b, padding=1)[0].permute(1, 2, 0)
    _close(conv64(F.pad(up, (0, 0, 1, 1, 1, 1)), w, b, 10, 12)[0], ref)
    # the phase form: output pixel (2 y + py, 2 x + px) = the 2x2 kernel of phase 2 py + px on source rows y - 1 + py + {0, 1} (the same in x).
    # phase_weights rounds to bf16; its fp64 form is rebuilt here from the same tap sets.
    rows = {0: ([0], [1, 2]), 1: ([0, 1], [2])}
    xp = F.pad(x, (0, 0, 1, 1, 1, 1))
    out = torch.zeros(10, 12, 4, dtype=torch.float64)
    for py in (0, 1):
        for px in (0, 1):
            w2 = torch.zeros(4, 8, 2, 2, dtype=torch.float64)
            for ty in (0, 1):
                for tx in (0, 1):
                    for a in rows[py][ty]:
                        for c in rows[px][tx]:
                            w2[:, :, ty, tx] += w[:, :, a, c]
            out[py::2, px::2] = conv64(xp, w2, b, 5, 6, oy=py, ox=px)[0]
    _close(out, ref)
    # and phase_weights' layout [phase][Cout][ty][tx][Cin] holds those kernels (bf16-exact inputs: small integers)
    wi = torch.randint(-3, 4, (4, 64, 3, 3)).double()
    w4 = phase_weights(wi.permute(0, 2, 3, 1).reshape(4, 9 * 64).bfloat16(), 64).double().view(4, 4, 2, 2, 64)
    xi = torch.randint(-3, 4, (5, 6, 64)).double()
    out = torch.zeros(10, 12, 4, dtype=torch.float64)
    for ph in range(4):
        out[ph >> 1::2, ph & 1::2] = conv64(F.pad(xi, (0, 0, 1, 1, 1, 1)), w4[ph].permute(0, 3, 1, 2), None, 5, 6, oy=ph >> 1, ox=ph & 1)[0]
    assert torch.equal(out, F.conv2d(F.interpolate(_nchw(xi), scale_factor=2, mode='nearest'), wi, None, padding=1)[0].permute(1, 2, 0))


def test_layer_table_covers_the_released_models():
    """Every 3x3 kernel of the released encoders (kl_encoder_shapes / qwen_encoder_shapes) and decoders (the state dicts the decoders' constructors load:
    oracle/vae_ref.py and oracle/vae_qwen_ref.py at the released widths) appears in CONV_CASES of tests/test_hip_vae_fp64.py with the channel counts the
    kernels run it at: inputs padded to a multiple of 64, outputs likewise except the decoders' 3 image channels (8) and the encoders' 32 moments."""
    from arcflow_amd.vae import kl_encoder_shapes, qwen_encoder_shapes
    from oracle import vae_qwen_ref, vae_ref
    from test_hip_vae_fp64 import CONV_CASES
    have = {(c[3], c[4]) for c in CONV_CASES if c[0] != 'ragged'}
    pad = lambda c: max(64, (c + 63) // 64 * 64)       # noqa: E731
    shapes = [kl_encoder_shapes(), qwen_encoder_shapes(),
              {k: tuple(v.shape) for k, v in vae_ref.make_decoder_weights((128, 256, 512, 512)).items()},
              {k: tuple(v.shape) for k, v in vae_qwen_ref.make_decoder_weights(dim=96).items()}]
    want = set()
    for sh in shapes:
        for k, s in sh.items():
            if k.endswith('.weight') and len(s) >= 4 and s[-1] == 3 and 'time_conv' not in k:
                ci = 3 if k == 'encoder.conv_in.weight' else pad(s[1])      # the image itself: afx_image_to_cols27 + the K = 64 GEMM
                want.add((ci, 8 if s[0] == 3 else 32 if s[0] == 32 else pad(s[0])))
    assert len(want) >= 16 and want <= have, sorted(want - have)
