"""The fp64 restatements of tests/masked_score_ref.py against the unmasked definitions they extend, the host formulas
``masked_metrics_from_sums`` / ``masked_ssim_from_sums`` on hand-made sums, ``student_edit_sigmas`` and the ``eval_cfg`` edit keys.  No GPU.
"""
import math

import pytest
import torch

import masked_score_ref as MR
import ssim_ref as SR

U = 2.0 ** -53


def _pair(shape, seed, dtype=torch.float32):
    g = torch.Generator().manual_seed(seed)
    b = torch.randn(shape, generator=g)
    a = 0.8 * b + 0.6 * torch.randn(shape, generator=g) + 0.05
    return a.to(dtype), b.to(dtype)


@pytest.mark.parametrize('transform', [False, True])
def test_masked_sums_reduce_to_the_unmasked_sums_and_to_zero(transform):
    a, b = _pair((2, 5, 64), 1)
    x = (SR.unit_range(a) if transform else a).double().flatten(1)
    y = (SR.unit_range(b) if transform else b).double().flatten(1)
    plain = torch.stack([((x - y) ** 2).sum(1), (x * x).sum(1), (y * y).sum(1), (x * y).sum(1)], 1)
    ones, mag = MR.masked_sums(a, b, torch.ones(2, 5, 4), (1, 5, 64), transform)
    assert torch.equal(ones[:, 0, 1:], plain) and (ones[:, 0, 0] == 320).all() and (ones[:, 1] == 0).all()
    zeros, _ = MR.masked_sums(a, b, torch.zeros(1, 5, 4), (1, 5, 64), transform)
    assert (zeros[:, 0] == 0).all() and torch.equal(zeros[:, 1, 1:], plain) and (zeros[:, 1, 0] == 320).all()
    # the two regions add up to the whole, for a fractional mask, within the roundings of the weighted terms
    m = MR.random_mask((2, 5, 4), 3)
    s, mag = MR.masked_sums(a, b, m, (1, 5, 64), transform)
    assert ((s[:, 0, 1:] + s[:, 1, 1:] - plain).abs() <= 4 * 320 * U * (mag[:, 0, 1:] + mag[:, 1, 1:])).all()
    assert ((s[:, 0, 0] + s[:, 1, 0] - 320).abs() <= 320 * U * 320).all()


def test_the_latent_weight_map_is_the_edit_blend_map_and_the_image_map_is_per_pixel():
    """Element e of token t reads m[t, e & 3]; channel (c, y, x) of an image reads m[y, x]; a batch of one is shared; the mutations move."""
    m = MR.random_mask((2, 3, 4), 5)
    w = MR.weights(m, 2, 1, 3, 64).view(2, 3, 64)
    for e in range(64):
        assert torch.equal(w[:, :, e], m[:, :, e & 3].double())
    assert not torch.equal(MR.weights(m, 2, 1, 3, 64, swap_hw=True), w.view(2, -1))
    assert torch.equal(MR.weights(m, 2, 1, 3, 64, swap_hw=True).view(2, 3, 64)[:, :, 1], m[:, :, 2].double())
    assert torch.equal(MR.weights(m, 2, 1, 3, 64, ignore_batch=True)[1], w[0].reshape(-1))
    mi = MR.random_mask((1, 1, 4, 6), 6)
    a = torch.zeros(2, 3, 4, 6)
    view, flat = MR.view_of(a, mi)
    assert view == (3, 24, 1) and flat.shape == (1, 24, 1)
    wi = MR.weights(flat, 2, *view).view(2, 3, 4, 6)
    assert torch.equal(wi, mi.double().expand(2, 3, 4, 6))
    s, _ = MR.masked_sums(*_pair((2, 3, 4, 6), 7), flat, view)
    t, _ = MR.masked_sums(*_pair((2, 3, 4, 6), 7), flat, view, swap_regions=True)
    assert torch.equal(s[:, 0], t[:, 1]) and torch.equal(s[:, 1], t[:, 0])


def test_masked_ssim_reduces_to_the_unmasked_mean_and_to_zero():
    shape = (2, 3, 12, 43)
    a, b = SR.make_inputs(*shape, 'fp32', 'noisy', True)
    mean = SR.ssim_mean(a, b, True, 1.0)
    n_win = 3 * 2 * 33
    ones = MR.masked_ssim_sums(a, b, torch.ones(1, 1, 12, 43), True, 1.0)
    assert ((ones[:, 0] / ones[:, 1] - mean).abs() <= 64 * U).all()           # the taps sum to 1 within a few ulp, then clamped: w = 1 - O(u)
    assert ((ones[:, 1] - n_win).abs() <= 64 * U * n_win).all() and (ones[:, 3].abs() <= 64 * U * n_win).all()
    zeros = MR.masked_ssim_sums(a, b, torch.zeros(2, 1, 12, 43), True, 1.0)
    assert (zeros[:, 0] == 0).all() and (zeros[:, 1] == 0).all() and (zeros[:, 3] == n_win).all()
    assert ((zeros[:, 2] / zeros[:, 3] - mean).abs() <= 64 * U).all()
    # a == b: every window is 1 (to rounding in this reference), so both means are 1
    m = MR.random_mask((2, 1, 12, 43), 8)
    rep, keep = MR.masked_ssim_means(a, a, m, True, 1.0)
    assert ((rep - 1).abs() <= 1e-12).all() and ((keep - 1).abs() <= 1e-12).all()
    # the window weight is the Gaussian mean over the window, not the centre value; a transposed mask is another mask
    sq = MR.random_mask((1, 1, 27, 27), 9)
    aa, bb = SR.make_inputs(1, 3, 27, 27, 'fp32', 'noisy', True)
    base = MR.masked_ssim_means(aa, bb, sq, True, 1.0)[0]
    assert (MR.masked_ssim_means(aa, bb, sq, True, 1.0, centre=True)[0] - base).abs().min() > 1e-6
    assert (MR.masked_ssim_means(aa, bb, sq, True, 1.0, transpose=True)[0] - base).abs().min() > 1e-6


def test_masked_host_formulas_on_hand_made_sums_and_the_empty_region():
    from arcflow_amd.train.evaluate import masked_metrics_from_sums, masked_ssim_from_sums, metrics_from_sums
    #            S_w  S_dd  S_aa  S_bb  S_ab
    sums = torch.tensor([[[8.0, 2.0, 2.0, 8.0, 3.0], [0.0, 0.0, 0.0, 0.0, 0.0]],
                         [[2.5, 0.0, 9.0, 9.0, 9.0], [5.5, 11.0, 1.0, 4.0, -2.0]]], dtype=torch.float64)
    rep, keep = masked_metrics_from_sums(sums, data_range=1.0)
    assert rep['weight'].tolist() == [8.0, 2.5] and keep['weight'].tolist() == [0.0, 5.5]
    assert rep['mse'].tolist() == [0.25, 0.0] and keep['mse'][1].item() == 2.0
    assert rep['rel_l2'].tolist() == [0.5, 0.0] and rep['cosine'].tolist() == [0.75, 1.0]
    assert abs(keep['rel_l2'][1].item() - math.sqrt(11.0 / 4.0)) < 1e-15 and keep['cosine'][1].item() == -1.0
    assert abs(rep['psnr'][0].item() - 10 * math.log10(4.0)) < 1e-12 and rep['psnr'][1].item() == 300.0        # the floor of metrics_from_sums
    for k in ('mse', 'rel_l2', 'cosine', 'psnr'):
        assert math.isnan(keep[k][0].item()) and not math.isnan(keep[k][1].item()), k
    # the last four sums with the weight as n are metrics_from_sums' own numbers
    plain = metrics_from_sums(sums[:, 0, 1:], 8, data_range=1.0)
    assert plain['mse'][0].item() == rep['mse'][0].item() and plain['cosine'][0].item() == rep['cosine'][0].item()
    assert 'psnr' not in masked_metrics_from_sums(sums)[0]
    rep_s, keep_s = masked_ssim_from_sums(torch.tensor([[3.0, 4.0, 1.0, 2.0], [0.0, 0.0, 5.0, 5.0], [2.0, 2.0, 0.0, 0.0]], dtype=torch.float64))
    assert rep_s[0].item() == 0.75 and keep_s[0].item() == 0.5 and math.isnan(rep_s[1].item()) and keep_s[1].item() == 1.0
    assert rep_s[2].item() == 1.0 and math.isnan(keep_s[2].item())


def test_student_edit_sigmas_and_the_named_masks():
    from arcflow_amd.schedule import mask_to_tokens, student_edit_sigmas, student_sigmas
    from arcflow_amd.train.evaluate import edit_mask
    for nfe, ratio in ((1, 1.0), (2, 1.0), (2, 0.5), (4, 0.5)):
        assert student_edit_sigmas(nfe, 128, ratio, 3.2, 1.0) == student_sigmas(nfe, 128, ratio, 3.2)
    full, part = student_sigmas(2, 128, 1.0, 3.2), student_edit_sigmas(2, 128, 1.0, 3.2, 0.6)
    assert len(part) == 3 and part[-1] == 0.0 and part[0] > part[1] > 0 and part[0] < full[0] and part[1] < full[1]
    assert abs(part[0] - 3.2 * 0.6 / (1 + 2.2 * 0.6)) < 1e-6                  # the static shift of the raw time `strength`
    with pytest.raises(ValueError):
        student_edit_sigmas(2, 128, 1.0, 3.2, 0.0)
    box, left = edit_mask('box', 2, 4, 6), edit_mask('left', 1, 4, 6)
    assert box.shape == (2, 1, 64, 96) and box.sum().item() == 2 * 32 * 48 and box[0, 0, 16, 24] == 1 and box[0, 0, 15, 24] == 0 and box[0, 0, 47, 71] == 1
    assert left.shape == (1, 1, 64, 96) and (left[..., :48] == 1).all() and (left[..., 48:] == 0).all()
    assert set(mask_to_tokens(box, 4, 6).unique().tolist()) == {0.0, 1.0}
    with pytest.raises(ValueError):
        edit_mask('ring', 1, 4, 6)


def test_eval_cfg_takes_the_edit_keys_and_a_config_without_them_reads_as_before():
    import os
    from arcflow_amd.train import config as CFG
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    cfg = CFG.load_config(os.path.join(root, 'examples', 'flux_distill_2nfe.py'))
    assert CFG.distill_setup(cfg)[3]['eval_cfg'] == CFG.EVAL_CFG_DEFAULTS and 'edit_mask' not in CFG.EVAL_CFG_DEFAULTS
    run = CFG.distill_setup(CFG.apply_options(cfg, {'eval_cfg': dict(edit_mask='box', edit_strength=0.6)}))[3]
    assert run['eval_cfg']['edit_mask'] == 'box' and run['eval_cfg']['edit_strength'] == 0.6 and run['eval_cfg']['teacher_steps'] == 28
    with pytest.raises(ValueError, match='edit_mask'):
        CFG.distill_setup(CFG.apply_options(cfg, {'eval_cfg': dict(edit_mask='ring')}))
    with pytest.raises(ValueError, match='edit_strength'):
        CFG.distill_setup(CFG.apply_options(cfg, {'eval_cfg': dict(edit_mask='left', edit_strength=1.5)}))
