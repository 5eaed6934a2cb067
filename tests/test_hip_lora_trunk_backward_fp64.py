"""The LoRA trunk's block backward (arcflow_amd/train/trunk.py: `_double_backward`, `_single_backward`, their `_from_stash` / `_recompute`
operand builders, `_adapted_backward`, and the chain `backward_sample`) per row, column and modulation slice against fp64 autograd, at the
released width (D = 3072, 24 heads; FLUX 2 + 2 blocks, Qwen-Image 2 blocks whose last one has an un-adapted text MLP).  The kernels have
per-element fp64 tests; their composition into a gradient was reached only through whole train steps at D = 256 with one block of a kind
and one rel-L2 per adapter tensor (test_distill.py, < 8e-2), which at this width never runs `_skinny`'s split-K branch, the [W | B] /
[W^T ; B^T] GEMMs at 3072 + rp columns, `s{i}.fused` with its adapter at row0 = 3 D or a second block's m0 / stash index, and cannot see
one lost row of dB, a mask drawn at the wrong global row, a d_gate from the other ybuf slot or one row of dX with the other stream's scale
(tests/lora_block_grad_ref.py).

Per case: one `student_forward_unmerged` (LoRA dropout 0.05, B != 0, one sigma per sample); then for every block and the LAST sample
(row0 != 0 where B > 1) the block's backward from its OWN input ckpt[block] with a seeded bf16 dXo into a zeroed gradient buffer and a
zeroed dmod -- nothing compounds.  Judged against
  * g64      fp64 autograd through mmdit_block_ref.block64 (LoRA branch, device masks, the modulation slice as a leaf),
  * g_eager  autograd through oracle/dit_ref.py's block under eager_bf16() from the same leaves,
with the standing bar: in every group -- dX increment rows / columns per stream, the dmod slices, every adapter's dA and dB
rows and columns -- the trunk's worst is at most 1.5 x the eager evaluation's worst.  Adapters of other blocks and dmod outside the block's
slice stay exactly zero.  The chain tests call `backward_sample` itself (norm_out's modulate, the dX hand-off, the dmod layout across blocks,
ckpt indexing) against the same two evaluations of the whole chain from the first block's input.  Measured ratios: DESIGN.md section 2
(printed here with -s).  The eager evaluation's dX carries the one bf16 rounding the dX hand-off between blocks has in the trunk AND in the
reference's own chain (lora_block_grad_ref.evaluate, round_dx): without it the first run's dX column maxima of six FLUX blocks stood at
1.5 - 2.0 x the eager evaluation's, exactly on the floor that rounding the fp64 dX to bf16 alone gives (printed per block).

Shapes (S = N + T rows per sample), the smallest that reach each branch:
  flux B 2, 16 x 16, T 77, S 333, r 256   ragged tiles in both streams; full stash, outputs-only stash (keep_xd = False), recompute
  flux B 1, 32 x 34, T 77, r 256          1088 image rows > 1024: `_skinny` at split_k = 8 (the case above takes 16)
  flux B 2, 12 x 16, T 64, S 256, r 48    rp = 64 != r: the zero-padded a16p
  flux B 2, 16 x 16, T 77, _LORA_TN off   the transposes + NT weight-gradient path a mis-aligned gradient slice falls back to
  qwen B 2,  8 x 14, T 45, r 256          full stash and recompute; the un-adapted txt MLP of the last block (the wt[...] dgrad branch)
"""
import re

import pytest
import torch

import lora_block_grad_ref as G
import mmdit_block_ref as R

pytestmark = pytest.mark.gpu

D_MODEL, HEADS, BAR, P_DROP, SEED = 3072, 24, 1.5, 0.05, 1234567
SIGMAS = [0.7619, 0.3]                        # one per sample: every sample has its own modulation vectors

# (family, B, hp, wp, T, rank, stash level, _LORA_TN)
CASES = [
    ('flux', 2, 16, 16, 77, 256, 'full', True),
    ('flux', 2, 16, 16, 77, 256, 'outputs', True),
    ('flux', 2, 16, 16, 77, 256, 'recompute', True),
    ('flux', 1, 32, 34, 77, 256, 'full', True),
    ('flux', 2, 12, 16, 64, 48, 'full', True),
    ('flux', 2, 16, 16, 77, 256, 'full', False),
    ('qwen', 2, 8, 14, 45, 256, 'full', True),
    ('qwen', 2, 8, 14, 45, 256, 'recompute', True),
]
CHAIN_CASES = [CASES[0], CASES[6]]
TEETH_CASES = [CASES[0], CASES[6]]

_WEIGHTS, _DISTS, _RUNS, _CHAINS = {}, {}, {}, {}


def _name(case):
    family, B, hp, wp, T, r, level, tn = case
    return f'{family} B={B} {hp}x{wp} T={T} r={r} {level}' + ('' if tn else ' no-TN')


def _weights(family):
    """(cfg, diffusers-named weights on the device with the teacher's and the student's heads): drawn once per module."""
    if family not in _WEIGHTS:
        from oracle import dit_ref
        if family == 'flux':
            cfg = dit_ref.FluxCfg(num_layers=2, num_single_layers=2)
            w = dit_ref.make_flux_weights(cfg, seed=31, teacher_head=True, device='cuda')
        else:
            cfg = dit_ref.QwenCfg(num_layers=2)
            w = dit_ref.make_qwen_weights(cfg, seed=32, device='cuda')
            g = torch.Generator(device='cuda').manual_seed(33)
            w['proj_out.weight'] = (torch.randn(64, D_MODEL, generator=g, device='cuda') * 0.05).bfloat16()
            w['proj_out.bias'] = (torch.randn(64, generator=g, device='cuda') * 0.02).bfloat16()
        assert cfg.dim == D_MODEL and cfg.heads == HEADS
        _WEIGHTS[family] = (cfg, w)
    return _WEIGHTS[family]


def _blocks(family):
    if family == 'qwen':
        return [('qwen', f'transformer_blocks.{i}.') for i in range(2)]
    return [('flux_double', f'transformer_blocks.{i}.') for i in range(2)] + [('flux_single', f'single_transformer_blocks.{i}.') for i in range(2)]


def _dist(family, rank, level):
    """One distiller per (family, rank, stash level); B != 0 (std 0.02)."""
    key = (family, rank, level)
    if key not in _DISTS:
        from arcflow_amd.train import ArcFlowDistiller, DistillConfig
        cfg, w = _weights(family)
        dc = DistillConfig(num_decay_iters=4, warmup_iters=0, grad_clip_begin_iter=10 ** 9, ema_start_iter=0, lora_rank=rank, lora_dropout=P_DROP)
        arch = dict(num_double=2, num_single=2) if family == 'flux' else dict(num_double=2, joint_dim=cfg.joint_dim)
        dist = ArcFlowDistiller(family, arch, w, dc)
        tr = dist.trunk
        tr.use_stash = level != 'recompute'
        tr.keep_xd = level == 'full'
        g = torch.Generator(device='cuda').manual_seed(41)
        for sp in tr.specs:
            tr.B(sp).copy_(torch.randn(sp.out_f, rank, generator=g, device='cuda') * 0.02)
        tr.refresh()
        assert tr.rp == (rank + 63) // 64 * 64 and len(tr.specs) == (14 if family == 'flux' else 8)
        _DISTS[key] = dist
    return _DISTS[key]


def _forward(case):
    """One training forward of the case; returns what the block backwards need."""
    family, B, hp, wp, T, rank, level, _ = case
    cfg, w = _weights(family)
    dist = _dist(family, rank, level)
    tr = dist.trunk
    N = hp * wp
    g = torch.Generator(device='cuda').manual_seed(1000 * B + T + rank)
    x = torch.randn(B, N, 64, generator=g, device='cuda')
    cond = dict(prompt_embeds=(torch.randn(B, T, cfg.joint_dim, generator=g, device='cuda') * 0.5).bfloat16(), hp=hp, wp=wp)
    if family == 'flux':
        cond['pooled'] = (torch.randn(B, cfg.pooled_dim, generator=g, device='cuda') * 0.5).bfloat16()
    sigma = torch.tensor(SIGMAS[:B], device='cuda')
    _, mod_all = dist.student_forward_unmerged(x, sigma, cond, P_DROP, SEED)
    torch.cuda.synchronize()
    assert (tr.stash is not None) == (level != 'recompute')
    if tr.stash is not None:
        assert tr.stash.keep_xd == (level == 'full')
    assert torch.isfinite(mod_all).all()
    if B > 1:
        assert (mod_all[0] - mod_all[1]).abs().max().item() > 1e-2
    return dist, w, mod_all, g


def _lora_leaves(tr, ads, row0, T, S):
    """{name: (a16, b16, keep_scale)}: the trunk's bf16 working copies and the DEVICE's masks, drawn as LoraTrunk._keep_scale draws them at
    the sample's global first row plus the stream's row offset."""
    from arcflow_amd import ops
    by_name = {sp.name: sp for sp in tr.specs}
    lora = {}
    for name, stream in ads:
        sp, rows = by_name[name], G.stream_rows(stream, T, S)
        ones = torch.ones(rows.stop - rows.start, sp.in_f, dtype=torch.bfloat16, device='cuda')
        keep = ops.lora_dropout(ones, P_DROP, tr._site_seed(sp), row0 + rows.start, mode=1) > 0
        lora[name] = (tr.a16[name], tr.b16[name], keep.float() / (1.0 - P_DROP))
    return lora


def _offsets(family):
    """((kind, prefix, offset of the block's slice in the modulation vector), ...), and the offset of norm_out's (scale, shift)."""
    out, m0 = [], 0
    for kind, p in _blocks(family):
        out.append((kind, p, m0))
        m0 += G.mod_size(kind, D_MODEL)
    return out, m0


def _slices(blocks):
    return [(f'{p}{nm}' if len(blocks) > 1 else nm, m0 + i * D_MODEL, m0 + (i + 1) * D_MODEL)
            for kind, p, m0 in blocks for i, nm in enumerate(G.slice_names(kind))]


def _run(case, monkeypatch=None):
    """Per block of the case: the errors of the trunk's backward and of the eager evaluation against fp64.  Computed once per case."""
    if case in _RUNS:
        return _RUNS[case]
    from arcflow_amd.train import trunk as trunk_mod
    family, B, hp, wp, T, rank, level, tn = case
    if not tn:
        monkeypatch.setattr(trunk_mod, '_LORA_TN', False)
    dist, w, mod_all, g = _forward(case)
    tr = dist.trunk
    N, S, nd = hp * wp, hp * wp + T, tr.nd
    b = B - 1
    row0 = b * S
    mod = mod_all[b]
    cos, sin = tr.eng.rope_tables(hp, wp, T)
    st = tr.stash if tr.use_stash else None
    offs, fin = _offsets(family)
    assert fin + 2 * D_MODEL == mod.numel()
    recs = []
    for blk, (kind, p, m0) in enumerate(offs):
        n_mod = G.mod_size(kind, D_MODEL)
        tr.row0 = row0
        tr.dmod = torch.zeros(mod.numel(), dtype=torch.float32, device='cuda')
        grads = torch.zeros_like(dist.grad)
        X = dist._ckpt[blk, row0:row0 + S]
        dXo = torch.randn(S, D_MODEL, generator=g, device='cuda').bfloat16()
        if blk < nd:
            dm = tr._double_mod(blk, mod)
            assert dm[0] == m0
            sv = tr._double_from_stash(blk, st, dm, cos, sin, T, S) if st is not None else tr._double_recompute(blk, X, dm, cos, sin, T)
            dX = tr._double_backward(blk, X, dm, cos, sin, T, sv, dXo, grads)
        else:
            sm = tr._single_mod(blk - nd, mod)
            assert sm[0] == m0
            sv = tr._single_from_stash(blk - nd, st, X, sm, cos, sin, T) if st is not None else tr._single_recompute(blk - nd, X, sm, cos, sin, T)
            dX = tr._single_backward(blk - nd, X, sm, cos, sin, T, sv, dXo, grads)
        del sv
        tr._join_wgrad()
        torch.cuda.synchronize()
        dmod, tr.dmod = tr.dmod, None
        txt_adapted = not (family == 'qwen' and blk == nd - 1)
        ads = G.block_adapters(kind, p, txt_adapted)
        by_name = {sp.name: sp for sp in tr.specs}
        got = dict(dX=dX, dmod=dmod[m0:m0 + n_mod], dA={n: tr.A(by_name[n], grads).clone() for n, _ in ads},
                   dB={n: tr.B(by_name[n], grads).clone() for n, _ in ads})
        # nothing else was touched: the other blocks' adapters, the embedder pair, the heads; dmod outside the block's slice
        a, z = tr.block_slice(blk)
        assert sorted(n for n, _ in ads) == sorted(sp.name for sp in tr.specs if a <= sp.off_a < z)
        assert not grads[:a].any() and not grads[z:].any() and grads[a:z].any()
        assert not dmod[:m0].any() and not dmod[m0 + n_mod:].any()
        lora = _lora_leaves(tr, ads, row0, T, S)
        tables = R.rope_tables(kind, hp, wp, T, 'cuda')
        one = [(kind, p, 0)]
        modb = mod[m0:m0 + n_mod]
        taps = [] if p.endswith('.1.') else None
        g64 = G.evaluate('fp64', one, w, HEADS, X, modb, lora, T, tables, dXo, taps=taps)
        ge = G.evaluate('eager', one, w, HEADS, X, modb, lora, T, tables, dXo)
        slices = _slices(one)
        # what the bf16 rounding of the fp64 dX alone costs per column (the floor under the trunk's and the eager evaluation's dX columns)
        floor = R.block_row_col_errors(dXo[None], g64['dX'].bfloat16()[None], g64['dX'][None], T)
        rec = dict(floor_cols=floor['cols'].max().item(), floor_rows=floor['rows'].max().item(), kind=kind, p=p, slices=slices, txt_adapted=txt_adapted, hip=G.grad_errors(got, g64, dXo, T, slices),
                   eager=G.grad_errors(ge, g64, dXo, T, slices), whole_hip=G.whole_rel_l2(got, g64), whole_eager=G.whole_rel_l2(ge, g64))
        if taps is not None and case in TEETH_CASES:          # the second block of each kind keeps what the teeth test plants into
            wrong = None
            if txt_adapted and kind != 'flux_single':         # the text stream's mlp1 mask drawn at the batch's first row, not the sample's
                n = [x for x, s in ads if s == 'txt'][0]
                other = dict(lora)
                k2 = _lora_leaves(tr, [(n, 'txt')], 0, T, S)[n][2]
                differs = ((k2 != lora[n][2]).sum(0) > 0)
                assert differs.any()
                other[n] = (lora[n][0], lora[n][1], k2)
                gw = G.evaluate('fp64', one, w, HEADS, X, modb, other, T, tables, dXo)
                wrong = (torch.where(differs[None], gw['dA'][n], g64['dA'][n]), gw['dX'])
            rec.update(g64={k: v for k, v in g64.items() if k != 'out'}, got=got, taps=taps, X=X.clone(), mod=modb.clone(), cot=dXo, wrong=wrong)
        recs.append(rec)
    _RUNS[case] = recs
    return recs


def _report(what, rec):
    ratios = G.assert_grads(rec['hip'], rec['eager'], BAR, rec['slices'], what)
    wh, we = rec['whole_hip'], rec['whole_eager']
    worst = max(wh, key=wh.get)
    print(f'{what}: hip max / eager max {G.format_ratios(ratios)}; worst {max(ratios.values()):.2f}; '
          f'whole-tensor rel-L2 dX hip {wh.get("dX", 0):.2e} eager {we.get("dX", 0):.2e}, dmod {wh["dmod"]:.2e} / {we["dmod"]:.2e}, '
          f'worst tensor {worst} {wh[worst]:.2e} / {we[worst]:.2e}' + (f'; bf16 rounding of the fp64 dX alone: worst row {rec["floor_rows"]:.2e} '
          f'(eager {rec["eager"]["dX"]["rows"].max().item():.2e}), worst column {rec["floor_cols"]:.2e} (eager {rec["eager"]["dX"]["cols"].max().item():.2e})' if 'floor_cols' in rec else ''))
    return ratios


@pytest.mark.parametrize('case', CASES, ids=_name)
def test_block_backward_per_row_column_and_slice_vs_fp64(case, monkeypatch):
    recs = _run(case, monkeypatch)
    failures = []
    for k, rec in enumerate(recs):
        what = f'{_name(case)} block {k} ({rec["p"][:-1]})'
        try:
            _report(what, rec)
        except AssertionError as e:           # (every block of the case is reported before the test fails)
            print(f'FAIL {e}')
            failures.append(str(e))
    assert not failures, '\n'.join(failures)


@pytest.mark.parametrize('case', TEETH_CASES, ids=_name)
def test_planted_faults_fail_the_check_on_the_trunks_gradients(case, monkeypatch):
    """The planted faults of test_lora_block_grad_ref_cpu.py on a copy of the TRUNK's gradients, the second block of each kind: each stays
    within 5e-2 of its whole tensor on top of the trunk's own error, and the check fails on it and names the place.  Reported: the
    smallest single-row scaling 1 + eps of a dX increment (last text row, first image row) the check detects."""
    T = case[4]
    for k, rec in enumerate(_run(case, monkeypatch)):
        if 'taps' not in rec:
            continue
        what = f'{_name(case)} block {k} ({rec["p"][:-1]})'
        for fault in G.FAULTS:
            if not G.fault_applies(fault, rec['kind'], rec['txt_adapted']):
                continue
            faulty, where, alphas = G.plant_fault(fault, rec['kind'], rec['p'], rec['g64'], rec['X'], rec['mod'], rec['cot'], T, rec['taps'],
                                                  rec['wrong'], rec['txt_adapted'], base=rec['got'])
            whole = G.whole_rel_l2(faulty, rec['g64'])
            assert all(whole[t] < 8e-2 for t in whole), (fault, whole)
            with pytest.raises(AssertionError) as ei:
                G.assert_grads(G.grad_errors(faulty, rec['g64'], rec['cot'], T, rec['slices']), rec['eager'], BAR, rec['slices'], what)
            assert re.search(where, str(ei.value)), (fault, where, str(ei.value))
            print(f'{what} {fault}: alpha {alphas}, whole-tensor rel-L2 {({t: round(whole[t], 4) for t in alphas})} (bound 8e-2), caught at /{where}/')
        eps = [G.smallest_detected_scaling(rec['got'], rec['g64'], rec['eager'], rec['cot'], T, row, BAR) for row in (T - 1, T)]
        print(f'{what}: smallest detected single-row scaling of the dX increment: text row {T - 1}: {eps[0]}, image row {T}: {eps[1]}')
        assert all(e is not None for e in eps), eps


def _chain(case):
    if case in _CHAINS:
        return _CHAINS[case]
    family, B, hp, wp, T, rank, level, _ = case
    dist, w, mod_all, g = _forward(case)
    tr = dist.trunk
    N, S = hp * wp, hp * wp + T
    b = B - 1
    row0 = b * S
    xf = torch.empty(B * N, D_MODEL, dtype=torch.bfloat16, device='cuda')
    dist.student.export('x_final', xf, B, N, T)
    dxn = torch.randn(N, D_MODEL, generator=g, device='cuda').bfloat16()
    grads = torch.zeros_like(dist.grad)
    dmod = torch.zeros(mod_all.shape[1], dtype=torch.float32, device='cuda')
    tr.backward_sample(dist._ckpt, b, mod_all, xf[b * N:(b + 1) * N], dxn, T, N, hp, wp, grads, dmod_out=dmod)
    torch.cuda.synchronize()
    tr.dmod = None
    offs, fin = _offsets(family)
    assert not dmod[fin:].any()               # (norm_out's own modulation gradient is the distiller's, not the trunk's)
    ads = [x for blk, (kind, p, _) in enumerate(offs) for x in G.block_adapters(kind, p, not (family == 'qwen' and blk == tr.nd - 1))]
    by_name = {sp.name: sp for sp in tr.specs}
    a, z = tr.block_slice(0)[0], tr.block_slice(len(offs) - 1)[1]
    assert not grads[:a].any() and not grads[z:].any()
    got = dict(dmod=dmod, dA={n: tr.A(by_name[n], grads) for n, _ in ads}, dB={n: tr.B(by_name[n], grads) for n, _ in ads})
    lora = _lora_leaves(tr, ads, row0, T, S)
    tables = R.rope_tables(offs[0][0], hp, wp, T, 'cuda')
    X = dist._ckpt[0, row0:row0 + S]
    g64 = G.evaluate('fp64', offs, w, HEADS, X, mod_all[b], lora, T, tables, dxn, final=fin)
    ge = G.evaluate('eager', offs, w, HEADS, X, mod_all[b], lora, T, tables, dxn, final=fin)
    # the reference's final tokens and the trunk's agree (the forward is tested elsewhere; here: x_final is this sample's rows)
    assert R.whole_rel_l2(xf[b * N:(b + 1) * N], g64['out'][T:]) < 2e-2
    slices = _slices(offs)                    # the blocks' slices: norm_out's pair is not the trunk's to fill
    rec = dict(slices=slices, hip=G.grad_errors(got, g64, None, T, slices, with_dx=False, zero_slices_exact=True),
               eager=G.grad_errors(ge, g64, None, T, slices, with_dx=False, zero_slices_exact=True))
    g64, ge = ({k: (v[:fin] if k == 'dmod' else v) for k, v in gs.items() if k not in ('dX', 'out')} for gs in (g64, ge))
    got['dmod'] = dmod[:fin]
    rec.update(whole_hip=G.whole_rel_l2(got, g64), whole_eager=G.whole_rel_l2(ge, g64))
    _CHAINS[case] = rec
    return rec


@pytest.mark.parametrize('case', CHAIN_CASES, ids=_name)
def test_backward_sample_chain_vs_fp64(case):
    """`backward_sample` for the last sample from a seeded dxn at the velocity head's input: norm_out's modulate (scale first, the `fin`
    offset), every block in reverse with the dX hand-off, the dmod layout across blocks, ckpt indexing -- against fp64 autograd through
    norm_out's modulate behind all the blocks, from the first block's input, and the eager-bf16 evaluation of the same chain."""
    _report(f'{_name(case)} chain', _chain(case))
