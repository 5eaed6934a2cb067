"""Prompt encoders (arcflow_amd/text_encoders.py) against the real transformers modules (fp32, CPU, random-init small
configs of the same architecture): T5 v1.1 encoder, CLIP text model, Qwen2.5-VL language model."""
import copy

import numpy as np
import pytest
import torch
from bf16_parity import U32, bf16_ulp, check_bf16, proj64
from splitk_ref import splitk_chunks, splitk_operands, splitk_ref

pytestmark = pytest.mark.gpu


def _rel(a, b):
    return ((a.float().cpu() - b.float()).norm() / b.float().norm()).item()


def _bf16_weights(m):
    # the engine holds bf16 weights: give the oracle the same (rounded) values
    with torch.no_grad():
        for p in m.parameters():
            p.copy_(p.bfloat16().float())
    return m


# (H, Hkv, head_dim, causal, relative-position bias): toy configurations, then the production encoders.  One whole-tensor rel-L2 per configuration, B = 1,
# packed rows: a smoke check.  The kernel is held per element against fp64 in test_hip_attention_ext_fp64.py.
_ATTN_TOY = [(4, 4, 64, False, True), (3, 3, 64, True, False), (8, 2, 128, True, False), (2, 2, 128, False, False)]
_T5_XXL, _CLIP_L, _QWEN25_LM = (64, 64, 64, False, True), (12, 12, 64, True, False), (28, 4, 128, True, False)


@pytest.mark.parametrize('S,configs', [pytest.param(64, _ATTN_TOY, id='64'), pytest.param(77, _ATTN_TOY, id='77'),
                                       pytest.param(200, _ATTN_TOY, id='200'), pytest.param(512, [_T5_XXL], id='t5xxl-512'),
                                       pytest.param(77, [_CLIP_L], id='clipl-77'), pytest.param(512, [_QWEN25_LM], id='qwen25-512'),
                                       pytest.param(333, [_QWEN25_LM], id='qwen25-333')])
def test_attention_ext_vs_torch(S, configs):
    import ctypes as C
    from arcflow_amd import _lib
    from arcflow_amd.text_encoders import _p, _s
    lib = _lib.load()
    g = torch.Generator().manual_seed(S)
    for (H, Hkv, d, causal, use_bias) in configs:
        Dq, Dk = H * d, Hkv * d
        qkv = (torch.randn(S, Dq + 2 * Dk, generator=g) * 0.7).bfloat16()
        scale = 1.0 if use_bias else d ** -0.5
        bias = (torch.randn(H, 2 * S - 1, generator=g)) if use_bias else None
        q = qkv[:, :Dq].double().view(S, H, d).transpose(0, 1)
        k = qkv[:, Dq:Dq + Dk].double().view(S, Hkv, d).transpose(0, 1).repeat_interleave(H // Hkv, 0)
        v = qkv[:, Dq + Dk:].double().view(S, Hkv, d).transpose(0, 1).repeat_interleave(H // Hkv, 0)
        s = q @ k.transpose(1, 2) * scale
        idx = torch.arange(S)
        if use_bias:
            s = s + bias.double()[:, (idx[None, :] - idx[:, None]) + S - 1]
        if causal:
            s = s.masked_fill(idx[None, :] > idx[:, None], float('-inf'))
        ref = (torch.softmax(s, -1) @ v).transpose(0, 1).reshape(S, Dq)
        qg = qkv.cuda()
        o = torch.empty(S, Dq, dtype=torch.bfloat16, device='cuda')
        ws = torch.empty(lib.afx_attention_ext_ws_bytes(1, Hkv, S, d), dtype=torch.uint8, device='cuda')
        ld = qg.stride(0)
        _lib.check(lib.afx_attention_ext_bf16(_p(qg), ld, _p(qg[:, Dq:]), ld, _p(qg[:, Dq + Dk:]), ld, _p(o), Dq, _p(ws), 1, H, Hkv, S, d,
                                              scale, int(causal), _p(None if bias is None else bias.cuda()), _s()))
        assert _rel(o, ref) < 1.5e-2, (H, Hkv, d, causal, use_bias, _rel(o, ref))



# ------------------------------------------------------------------------------------------ row kernels of afx_text.hip at the encoders' widths
# Against fp64 from the same bf16 inputs.  Element-wise kernels: every element within one bf16 ulp (+ the fp32 rounding of a sum that can
# cancel, where said) and >= 99 % equal to the reference rounded to nearest even -- a systematic relative error e shifts ~e / 5.4e-3 of the
# elements, so 3e-3 fails.  norm_rows: one bf16 ulp plus fp32 eps x D x the row's input scale (|x| rstd |w| + |b|), >= 98 % rounded like
# the reference: a 1e-3 error of rstd fails it.
def _text_lib():
    from arcflow_amd import _lib
    from arcflow_amd.text_encoders import _p, _s
    return _lib, _lib.load(), _p, _s


def _gen(seed):
    return torch.Generator(device='cuda').manual_seed(seed)


@pytest.mark.parametrize('D,rms,eps,offset', [(768, False, 1e-5, 0.0), (768, False, 1e-5, 80.0), (4096, True, 1e-6, 0.0), (3584, True, 1e-6, 0.0),
                                              (8192, True, 1e-6, 0.0), (8192, False, 1e-5, 0.0)])
def test_norm_rows_vs_fp64(D, rms, eps, offset):
    """LayerNorm (CLIP-L: 768, eps 1e-5, with bias) and RMSNorm (T5-XXL 4096, Qwen2.5 3584, eps 1e-6), the documented maximum D = 8192
    (16 chunks per lane), a row-strided input and output, and LayerNorm rows whose mean is 64x their standard deviation."""
    _lib, lib, _p, _s = _text_lib()
    R = 333
    g = _gen(D + int(rms) + int(offset))
    x = (torch.randn(R, D + 64, generator=g, device='cuda') * (1.0 if offset else 2.0) + (offset or 0.3)).bfloat16()[:, 32:32 + D]
    if offset:
        assert bool((x.double().mean(-1) >= 64 * x.double().std(-1)).all())
    w = (1 + 0.3 * torch.randn(D, generator=g, device='cuda')).bfloat16().float()
    b = None if rms else (0.5 * torch.randn(D, generator=g, device='cuda')).bfloat16().float()
    obuf = torch.full((R, D + 48), 3.0, dtype=torch.bfloat16, device='cuda')
    y = obuf[:, 8:8 + D]
    _lib.check(lib.afx_norm_rows_bf16(_p(x), x.stride(0), _p(y), y.stride(0), R, D, _p(w), _p(b), eps, int(rms), _s()))
    assert bool((obuf[:, :8] == 3.0).all() and (obuf[:, 8 + D:] == 3.0).all())
    xd = x.double()
    mean = 0.0 if rms else xd.mean(-1, keepdim=True)
    var = (xd * xd).mean(-1, keepdim=True) if rms else ((xd - mean) ** 2).mean(-1, keepdim=True)
    rstd = 1.0 / torch.sqrt(var + eps)
    ref = (xd - mean) * rstd * w.double() + (0.0 if b is None else b.double())
    row_scale = (xd.abs() * rstd * w.double().abs()).amax(-1, keepdim=True) + (0.0 if b is None else b.double().abs().max())
    check_bf16(y, ref, floor=U32 * D * row_scale, min_equal=0.98, what=f'norm_rows D={D} rms={rms} offset={offset}')


@pytest.mark.parametrize('F,act,gated', [(10240, 2, True), (18944, 1, True), (3072, 3, False)])
def test_act_mul_vs_fp64(F, act, gated):
    """T5-XXL's gated gelu-tanh (F = 10240, gate at column F), Qwen2.5's gated SiLU (18944) and CLIP's quick_gelu (3072), read from rows
    of stride 2F, written into a column view of a wider output."""
    _lib, lib, _p, _s = _text_lib()
    M = 256
    g = _gen(F + act)
    x = (torch.randn(M, 2 * F, generator=g, device='cuda') * 3).clamp(-9.5, 9.5).bfloat16()
    obuf = torch.full((M, F + 64), -2.0, dtype=torch.bfloat16, device='cuda')
    out = obuf[:, 32:32 + F]
    _lib.check(lib.afx_act_mul_bf16(_p(x), x.stride(0), _p(out), out.stride(0), M, F, F if gated else -1, act, _s()))
    assert bool((obuf[:, :32] == -2.0).all() and (obuf[:, 32 + F:] == -2.0).all())
    a = x[:, :F].double()
    if act == 1:
        r = a * torch.sigmoid(a)
    elif act == 2:
        r = a * torch.sigmoid(2 * (2.0 / np.pi) ** 0.5 * (a + 0.044715 * a ** 3))      # = 0.5 a (1 + tanh u), without fp64's cancellation for a < -5
    else:
        r = a * torch.sigmoid(1.702 * a)
    if gated:
        r = r * x[:, F:].double()
    check_bf16(out, r, what=f'act_mul F={F} act={act}')


def test_rope_half_qwen_row_in_place():
    """Rotate-half RoPE in place on the 28 q + 4 k heads of 128 of a Qwen2.5 qkv row (v's 4 heads follow and must come back untouched)."""
    _lib, lib, _p, _s = _text_lib()
    S, H, Hkv, d = 333, 28, 4, 128
    g = _gen(S)
    width = (H + 2 * Hkv) * d
    qkv = (torch.randn(S, width + 64, generator=g, device='cuda') + 0.1).bfloat16()
    before = qkv.clone()
    pos = torch.arange(S, device='cuda', dtype=torch.float64)[:, None]
    inv = 1.0 / (1e6 ** (torch.arange(0, d, 2, device='cuda', dtype=torch.float64) / d))
    ang = pos * inv[None]
    cos, sin = torch.cos(ang).float().contiguous(), torch.sin(ang).float().contiguous()
    view = qkv[:, :width]
    _lib.check(lib.afx_rope_half_bf16(_p(view), view.stride(0), _p(cos), _p(sin), S, H + Hkv, d, _s()))
    assert torch.equal(qkv[:, (H + Hkv) * d:], before[:, (H + Hkv) * d:])
    x = before[:, :(H + Hkv) * d].double().view(S, H + Hkv, d)
    a, b = x[..., :d // 2], x[..., d // 2:]
    c, s_ = cos.double()[:, None], sin.double()[:, None]
    ref = torch.cat([a * c - b * s_, b * c + a * s_], -1)
    # two products and a sum in fp32: where the sum cancels, their roundings (2 u of |a c| + |b s|) show
    floor = 2 * U32 * torch.cat([(a * c).abs() + (b * s_).abs(), (b * c).abs() + (a * s_).abs()], -1)
    check_bf16(qkv[:, :(H + Hkv) * d].view(S, H + Hkv, d), ref, floor=floor, what='rope_half')


@pytest.mark.parametrize('V,D,S,with_pos', [(32128, 4096, 512, False), (49408, 768, 77, True)])
def test_embed_rows_last_row(V, D, S, with_pos):
    """Embedding gather with ids that include the last vocabulary row: T5-XXL without positions (bit-exact copy), CLIP-L with its
    position table (one fp32 add, then the bf16 rounding)."""
    _lib, lib, _p, _s = _text_lib()
    g = _gen(V)
    table = torch.randn(V, D, generator=g, device='cuda').bfloat16()
    ids = torch.randint(0, V, (S,), generator=g, device='cuda', dtype=torch.int32)
    ids[0], ids[S // 2], ids[-1] = V - 1, 0, V - 1
    pos = (0.3 * torch.randn(S, D, generator=g, device='cuda')).bfloat16() if with_pos else None
    out = torch.empty(S, D, dtype=torch.bfloat16, device='cuda')
    _lib.check(lib.afx_embed_rows_bf16(_p(table), _p(ids), _p(pos), _p(out), S, D, _s()))
    rows = table[ids.long()]
    if pos is None:
        assert torch.equal(out, rows)
    else:
        check_bf16(out, rows.double() + pos.double(), what='embed_rows + pos')

def test_t5_encoder_vs_transformers():
    from transformers import T5Config, T5EncoderModel
    from arcflow_amd.text_encoders import T5Encoder, t5_relative_buckets
    torch.manual_seed(0)
    cfg = T5Config(vocab_size=300, d_model=128, d_kv=64, d_ff=256, num_layers=3, num_heads=4, feed_forward_proj='gated-gelu',
                   relative_attention_num_buckets=32, relative_attention_max_distance=128, dropout_rate=0.0)
    m = _bf16_weights(T5EncoderModel(cfg).eval())
    with torch.no_grad():      # default init leaves the bias table and norms trivial: make them matter
        for n, p in m.named_parameters():
            if 'relative_attention_bias' in n:
                p.copy_((torch.randn_like(p) * 0.5).bfloat16().float())
            if 'layer_norm' in n:
                p.copy_((1 + 0.2 * torch.randn_like(p)).bfloat16().float())
    # the bucket function against the module's own
    from transformers.models.t5.modeling_t5 import T5Attention
    d = torch.arange(-300, 301)
    assert torch.equal(t5_relative_buckets(d), T5Attention._relative_position_bucket(d, True, 32, 128))
    ids = torch.randint(0, 300, (2, 96))
    ids[1, 40:] = 0                                        # padding tokens are ordinary tokens (no mask is passed)
    with torch.no_grad():
        ref = m(input_ids=ids).last_hidden_state
    enc = T5Encoder(m.state_dict(), num_layers=3, num_heads=4, d_kv=64)
    out = enc(ids)
    assert out.shape == ref.shape and _rel(out, ref) < 2e-2, _rel(out, ref)


def test_clip_text_encoder_vs_transformers():
    from transformers import CLIPTextConfig, CLIPTextModel
    from arcflow_amd.text_encoders import CLIPTextEncoder
    torch.manual_seed(1)
    for eos_cfg in (2, 299):
        cfg = CLIPTextConfig(vocab_size=300, hidden_size=128, intermediate_size=256, num_hidden_layers=3, num_attention_heads=2,
                             max_position_embeddings=77, hidden_act='quick_gelu', eos_token_id=eos_cfg, bos_token_id=298, pad_token_id=299)
        m = _bf16_weights(CLIPTextModel(cfg).eval())
        ids = torch.randint(0, 290, (2, 77))
        ids[:, 0] = 298
        ids[0, 20:] = 299                                  # eos (= highest id) then padding with the same id
        ids[1, 50:] = 299
        with torch.no_grad():
            ref = m(input_ids=ids)
        enc = CLIPTextEncoder(m.state_dict(), num_layers=3, num_heads=2, eos_token_id=eos_cfg)
        hs, pooled = enc(ids)
        assert _rel(hs, ref.last_hidden_state) < 2e-2 and _rel(pooled, ref.pooler_output) < 2e-2


def test_qwen25_text_encoder_vs_transformers():
    from transformers import Qwen2_5_VLConfig, Qwen2_5_VLForConditionalGeneration
    from arcflow_amd.text_encoders import Qwen25TextEncoder
    torch.manual_seed(2)
    text = dict(vocab_size=400, hidden_size=256, intermediate_size=512, num_hidden_layers=3, num_attention_heads=2, num_key_value_heads=1,
                max_position_embeddings=512, rope_theta=1e6, rms_norm_eps=1e-6, tie_word_embeddings=False,
                rope_scaling=dict(type='mrope', mrope_section=[16, 24, 24]))
    vis = dict(depth=1, hidden_size=64, intermediate_size=128, num_heads=2, out_hidden_size=256)
    try:
        cfg = Qwen2_5_VLConfig(text_config=text, vision_config=vis)
    except TypeError:
        cfg = Qwen2_5_VLConfig(vision_config=vis, **text)
    m = _bf16_weights(Qwen2_5_VLForConditionalGeneration(cfg).eval())
    with torch.no_grad():
        for n, p in m.named_parameters():
            if 'layernorm' in n or n.endswith('norm.weight'):
                p.copy_((1 + 0.2 * torch.randn_like(p)).bfloat16().float())
            if n.endswith('proj.bias'):
                p.copy_((0.3 * torch.randn_like(p)).bfloat16().float())
    ids = torch.randint(0, 390, (2, 90))
    mask = torch.ones(2, 90, dtype=torch.long)
    mask[1, 70:] = 0
    with torch.no_grad():
        ref = m(input_ids=ids, attention_mask=mask, output_hidden_states=True).hidden_states[-1]
    enc = Qwen25TextEncoder(m.state_dict(), num_layers=3, num_heads=2, num_kv_heads=1)
    out = enc(ids, mask)
    assert _rel(out[0], ref[0]) < 2e-2, _rel(out[0], ref[0])
    assert _rel(out[1, :70], ref[1, :70]) < 2e-2


class _Tok:
    """Stand-in tokenizer (the real ones are transformers tokenizers read from the model snapshot): hashes characters to ids."""

    def __init__(self, vocab, pad_id, eos_id=None, bos_id=None, left_pad=False):
        self.vocab, self.pad, self.eos, self.bos, self.left = vocab, pad_id, eos_id, bos_id, left_pad

    def __call__(self, texts, padding=True, max_length=None, truncation=True, return_tensors='pt'):
        rows = []
        for t in texts:
            ids = [(ord(c) * 7) % (self.vocab - 10) for c in t]
            ids = ([self.bos] if self.bos is not None else []) + ids + ([self.eos] if self.eos is not None else [])
            rows.append(ids[:max_length])
        L = max_length if padding == 'max_length' else max(len(r) for r in rows)
        ids = torch.full((len(rows), L), self.pad, dtype=torch.long)
        mask = torch.zeros(len(rows), L, dtype=torch.long)
        for i, r in enumerate(rows):
            sl = slice(L - len(r), L) if self.left else slice(0, len(r))
            ids[i, sl] = torch.tensor(r)
            mask[i, sl] = 1
        return type('Enc', (), dict(input_ids=ids, attention_mask=mask))()


def test_qwen_encode_prompt_matches_transformers_path():
    """pipe.encode_prompt (template, valid-token extraction, 34-token drop, zero padding) with the HIP encoder vs the same
    host logic around the transformers module; a left-padding tokenizer checks the mask handling."""
    from transformers import Qwen2_5_VLConfig, Qwen2_5_VLForConditionalGeneration
    from arcflow_amd.pipelines import ArcQwenImagePipeline
    from arcflow_amd.text_encoders import Qwen25TextEncoder
    torch.manual_seed(3)
    text = dict(vocab_size=400, hidden_size=256, intermediate_size=512, num_hidden_layers=2, num_attention_heads=2, num_key_value_heads=1,
                max_position_embeddings=2048, rope_theta=1e6, rms_norm_eps=1e-6, tie_word_embeddings=False,
                rope_scaling=dict(type='mrope', mrope_section=[16, 24, 24]))
    cfg = Qwen2_5_VLConfig(text_config=text, vision_config=dict(depth=1, hidden_size=64, intermediate_size=128, num_heads=2, out_hidden_size=256))
    m = _bf16_weights(Qwen2_5_VLForConditionalGeneration(cfg).eval())
    prompts = ['a red cube on a glass table', 'two cats']
    for left in (False, True):
        pipe = ArcQwenImagePipeline()
        pipe.tokenizer = _Tok(400, pad_id=399, left_pad=left)
        pipe.text_encoder = Qwen25TextEncoder(m.state_dict(), num_layers=2, num_heads=2, num_kv_heads=1)
        emb, mask = pipe.encode_prompt(prompts)
        ref_pipe = ArcQwenImagePipeline()
        ref_pipe.tokenizer, ref_pipe.text_encoder = pipe.tokenizer, m
        with torch.no_grad():
            remb, rmask = ref_pipe.encode_prompt(prompts)
        assert emb.shape == remb.shape and torch.equal(mask.cpu(), rmask.cpu())
        assert mask.sum(1).tolist() == [len(pipe.prompt_template_encode.format(p)) - 34 for p in prompts]
        assert _rel(emb, remb) < 2e-2, (left, _rel(emb, remb))


def test_flux_encode_prompt_with_hip_encoders():
    from transformers import CLIPTextConfig, CLIPTextModel, T5Config, T5EncoderModel
    from arcflow_amd.pipelines import ArcFluxPipeline
    from arcflow_amd.text_encoders import CLIPTextEncoder, T5Encoder
    torch.manual_seed(4)
    t5 = _bf16_weights(T5EncoderModel(T5Config(vocab_size=300, d_model=128, d_kv=64, d_ff=256, num_layers=2, num_heads=2,
                                               feed_forward_proj='gated-gelu', dropout_rate=0.0)).eval())
    clip = _bf16_weights(CLIPTextModel(CLIPTextConfig(vocab_size=300, hidden_size=64, intermediate_size=128, num_hidden_layers=2, num_attention_heads=1,
                                                      max_position_embeddings=77, eos_token_id=2, bos_token_id=298, pad_token_id=299)).eval())
    pipe = ArcFluxPipeline()
    pipe.tokenizer, pipe.tokenizer_2 = _Tok(300, pad_id=299, eos_id=299, bos_id=298), _Tok(300, pad_id=0, eos_id=1)
    pipe.text_encoder = CLIPTextEncoder(clip.state_dict(), num_layers=2, num_heads=1, eos_token_id=2)
    pipe.text_encoder_2 = T5Encoder(t5.state_dict(), num_layers=2, num_heads=2, d_kv=64)
    pe, pooled = pipe.encode_prompt('a photo of a fox', None, None, None, 'cuda', 2, 128)
    with torch.no_grad():
        ids = pipe.tokenizer(['a photo of a fox'], padding='max_length', max_length=77).input_ids
        ids2 = pipe.tokenizer_2(['a photo of a fox'], padding='max_length', max_length=128).input_ids
        rp, re = clip(input_ids=ids).pooler_output, t5(input_ids=ids2).last_hidden_state
    assert pe.shape == (2, 128, 128) and pooled.shape == (2, 64)
    assert _rel(pe[0], re[0]) < 2e-2 and _rel(pooled[1], rp[0]) < 2e-2


def test_prompt_cache_round_trip_and_online_cond(tmp_path):
    """tools/cache_prompts.py path: prompts -> HIP encoders -> cache files -> PromptEmbedCache -> collate == online cond."""
    from transformers import CLIPTextConfig, CLIPTextModel, T5Config, T5EncoderModel
    from arcflow_amd.pipelines import ArcFluxPipeline
    from arcflow_amd.text_encoders import CLIPTextEncoder, T5Encoder
    from arcflow_amd.train import data as DATA
    from arcflow_amd.train.prompts import PromptEncoder, write_cache
    torch.manual_seed(5)
    t5 = _bf16_weights(T5EncoderModel(T5Config(vocab_size=300, d_model=128, d_kv=64, d_ff=256, num_layers=1, num_heads=2,
                                               feed_forward_proj='gated-gelu', dropout_rate=0.0)).eval())
    clip = _bf16_weights(CLIPTextModel(CLIPTextConfig(vocab_size=300, hidden_size=64, intermediate_size=128, num_hidden_layers=1, num_attention_heads=1,
                                                      max_position_embeddings=77, eos_token_id=2, bos_token_id=298, pad_token_id=299)).eval())
    pipe = ArcFluxPipeline()
    pipe.tokenizer, pipe.tokenizer_2 = _Tok(300, pad_id=299, eos_id=299, bos_id=298), _Tok(300, pad_id=0, eos_id=1)
    pipe.text_encoder = CLIPTextEncoder(clip.state_dict(), num_layers=1, num_heads=1, eos_token_id=2)
    pipe.text_encoder_2 = T5Encoder(t5.state_dict(), num_layers=1, num_heads=2, d_kv=64)
    enc = PromptEncoder('flux', pipe, max_sequence_length=64)
    prompts = ['a fox', 'two red cubes on a table', 'sunset']
    names = write_cache(enc, prompts, str(tmp_path / 'cache'), latent_size=(16, 16, 16), batch=2, compress=False)
    assert names == ['00000000', '00000001', '00000002'] and (tmp_path / 'cache.jsonl').exists()
    ds = DATA.PromptEmbedCache(str(tmp_path / 'cache'), pad_seq_len=64)
    assert len(ds) == 3 and ds[1]['name'] == prompts[1]
    batch = DATA.collate([ds[0], ds[1]], device='cuda')
    online = enc.cond(prompts[:2], 8, 8)
    assert (batch['hp'], batch['wp']) == (8, 8)
    assert _rel(batch['prompt_embeds'], online['prompt_embeds'].cpu()) < 4e-3          # fp16 storage of bf16 values
    assert _rel(batch['pooled'], online['pooled'].cpu()) < 4e-3


# ------------------------------------------------------------------------------------------ _linear at every released launch shape, per element
# Widths from the released configurations the tests above quote (T5 v1.1 XXL: d_model 4096, 64 heads of 64, d_ff 10240, gated; CLIP ViT-L/14 text:
# 768 / 3072, biases; Qwen2.5-VL-7B language model: 3584, 28 + 4 + 4 heads of 128 -> q|k|v 4608 with bias, gate|up 2 x 18944) and the stacking of
# text_encoders.py.  route: what _Base._linear does with the shape -- 'plain' (ops.linear), 8 / 16 (ops.linear_splitk with that many chunks asked
# for: K >= 8192) or 0 (ops.linear_splitk, automatic chunking: K >= 3072 and at most 80 tiles of 128 x 128).  A change of the rule changes this table.
# (encoder, site, M, N, K, bias, residual, route)
def _qwen_rows(S, qkv_o_route):
    return [('qwen', 'qkv', S, 4608, 3584, True, False, qkv_o_route), ('qwen', 'o', S, 3584, 3584, False, True, qkv_o_route),
            ('qwen', 'gate_up', S, 37888, 3584, False, False, 'plain'), ('qwen', 'down', S, 3584, 18944, False, True, 16)]


LINEAR_TABLE = [
    ('t5', 'qkv', 512, 12288, 4096, False, False, 'plain'), ('t5', 'o', 512, 4096, 4096, False, True, 'plain'),
    ('t5', 'wi', 512, 20480, 4096, False, False, 'plain'), ('t5', 'wo', 512, 4096, 10240, False, True, 8),
    ('clip', 'qkv', 77, 2304, 768, True, False, 'plain'), ('clip', 'out', 77, 768, 768, True, True, 'plain'),
    ('clip', 'fc1', 77, 3072, 768, True, False, 'plain'), ('clip', 'fc2', 77, 768, 3072, True, True, 0),
] + _qwen_rows(40, 0) + _qwen_rows(162, 0) + _qwen_rows(1058, 'plain')


@pytest.mark.parametrize('row', LINEAR_TABLE, ids=[f'{r[0]}-{r[1]}-{r[2]}' for r in LINEAR_TABLE])
def test_linear_rule_every_released_shape_vs_fp64(row, monkeypatch):
    """The encoders' own _linear on one released launch: the route it takes (recorded round ops.linear / ops.linear_splitk) and the result per
    element against fp64 with the bound of that route -- splitk_ref.py's for the split-K routes; proj64 (K / 32 + 33) for the plain ones, with the
    gate_res floor of test_hip_gemm_fp64.py (gate 1: + 2 u (|y| + |r|)) where a residual is added.  Teeth: K column K - 1 left out."""
    from arcflow_amd import ops
    from arcflow_amd.text_encoders import _Base
    enc, site, M, N, K, bias, res, route = row
    a, w, b, r = splitk_operands(M, N, K, bias, res, seed=M + N + K, device='cuda', draw_on='cuda')
    calls = []
    real_splitk, real_linear = ops.linear_splitk, ops.linear

    def rec_splitk(x, w_, b_=None, residual=None, out=None, split_k=0):
        calls.append(split_k)
        return real_splitk(x, w_, b_, residual, out=out, split_k=split_k)

    def rec_linear(*args, **kw):
        calls.append('plain')
        return real_linear(*args, **kw)
    monkeypatch.setattr(ops, 'linear_splitk', rec_splitk)
    monkeypatch.setattr(ops, 'linear', rec_linear)
    out = _Base('cuda')._linear(a, w, b, r)
    torch.cuda.synchronize()
    assert calls == [route], f'{enc} {site} {M}x{N}x{K}: _linear took {calls}, the table says {route}'
    what = f'_linear {enc} {site} {M}x{N}x{K} route={route}'
    if route == 'plain':
        y, fl = proj64(a, w, b)
        if r is not None:
            fl = fl + 2 * U32 * (y.abs() + r.double().abs())
            y = y + r.double()
    else:
        y, fl, _ = splitk_ref(a, w, b, r, splitk_chunks(M, N, K, route)[0])
    check_bf16(out, y, floor=fl, what=what)
    print(f'{what}: worst err / tol {((out.double() - y).abs() / (bf16_ulp(y) + fl)).max().item():.3f}')
    with pytest.raises(AssertionError, match='beyond one bf16 ulp'):
        check_bf16(out, y - a[:, K - 1].double()[:, None] * w[:, K - 1].double()[None, :], floor=fl, min_equal=0.0, what=f'{what}: one K column dropped')


# ------------------------------------------------------------------------------------------ one layer of each encoder at its released width
# The transformers module itself, one layer, a vocabulary of a few hundred, weights rounded to bf16: evaluated on the device in fp64 (the reference;
# the modules' own fp32 islands -- T5's norm variance and softmax -- stay fp32, 1e-7 against a bar of 1e-3) and as the eager bf16 module.  The bar
# is test_full_depth_parity.py's: rel-L2(hip, fp64) <= 1.5 x rel-L2(eager bf16, fp64) + 2e-3, per output.  At these widths _linear takes its
# split-K routes (T5 wo: K = 10240; Qwen down: 18944, q|k|v and o: automatic; CLIP fc2: 3072), which no toy configuration reaches.
FACTOR, FLOOR = 1.5, 2e-3


def _rel64(x, ref):
    return ((x.double() - ref.double()).norm() / ref.double().norm()).item()


def _layer_parity(name, m, run_module, run_hip):
    """run_module(module) -> tuple of outputs; run_hip() -> the same tuple from the HIP encoder.  Prints and asserts the bar per output."""
    m.config._attn_implementation = 'eager'
    m16 = copy.deepcopy(m).to('cuda', torch.bfloat16)
    hip = run_hip()
    m64 = m.to('cuda', torch.float64)
    with torch.no_grad():
        ref, eag = run_module(m64), run_module(m16)
    for i, (h, r64, e16) in enumerate(zip(hip, ref, eag)):
        eh, ee = _rel64(h, r64), _rel64(e16, r64)
        print(f'{name} output {i}: rel-L2 hip {eh:.3e}, eager bf16 {ee:.3e}')
        assert eh <= FACTOR * ee + FLOOR, (name, i, eh, ee)


def test_t5_xxl_one_layer_vs_fp64():
    from transformers import T5Config, T5EncoderModel
    from arcflow_amd.text_encoders import T5Encoder
    torch.manual_seed(10)
    cfg = T5Config(vocab_size=300, d_model=4096, d_kv=64, d_ff=10240, num_layers=1, num_heads=64, feed_forward_proj='gated-gelu',
                   relative_attention_num_buckets=32, relative_attention_max_distance=128, dropout_rate=0.0)
    m = T5EncoderModel(cfg).eval()
    with torch.no_grad():
        for n, p in m.named_parameters():
            if 'relative_attention_bias' in n:
                p.copy_(torch.randn_like(p) * 0.5)
            if 'layer_norm' in n:
                p.copy_(1 + 0.2 * torch.randn_like(p))
    m = _bf16_weights(m)
    ids = torch.randint(0, 300, (1, 512))
    enc = T5Encoder(m.state_dict(), num_layers=1, num_heads=64, d_kv=64)
    _layer_parity('t5-xxl 1 layer S=512', m, lambda mod: (mod(input_ids=ids.cuda()).last_hidden_state[0],), lambda: (enc(ids)[0],))


def test_clip_l_one_layer_vs_fp64():
    from transformers import CLIPTextConfig, CLIPTextModel
    from arcflow_amd.text_encoders import CLIPTextEncoder
    torch.manual_seed(11)
    cfg = CLIPTextConfig(vocab_size=300, hidden_size=768, intermediate_size=3072, num_hidden_layers=1, num_attention_heads=12,
                         max_position_embeddings=77, hidden_act='quick_gelu', eos_token_id=2, bos_token_id=298, pad_token_id=299)
    m = CLIPTextModel(cfg).eval()
    with torch.no_grad():
        for n, p in m.named_parameters():
            if 'layer_norm' in n and n.endswith('weight'):
                p.copy_(1 + 0.2 * torch.randn_like(p))
            if n.endswith('bias'):
                p.copy_(0.3 * torch.randn_like(p))
    m = _bf16_weights(m)
    ids = torch.randint(0, 290, (1, 77))
    ids[0, 0], ids[0, 30:] = 298, 299
    enc = CLIPTextEncoder(m.state_dict(), num_layers=1, num_heads=12, eos_token_id=2)

    def run_module(mod):
        o = mod(input_ids=ids.cuda())
        return o.last_hidden_state[0], o.pooler_output[0]

    def run_hip():
        hs, pooled = enc(ids)
        return hs[0], pooled[0]
    _layer_parity('clip-l 1 layer S=77', m, run_module, run_hip)


def test_qwen25_7b_one_layer_vs_fp64():
    from transformers import Qwen2_5_VLConfig, Qwen2_5_VLForConditionalGeneration
    from arcflow_amd.text_encoders import Qwen25TextEncoder
    torch.manual_seed(12)
    text = dict(vocab_size=400, hidden_size=3584, intermediate_size=18944, num_hidden_layers=1, num_attention_heads=28, num_key_value_heads=4,
                max_position_embeddings=2048, rope_theta=1e6, rms_norm_eps=1e-6, tie_word_embeddings=False,
                rope_scaling=dict(type='mrope', mrope_section=[16, 24, 24]))
    vis = dict(depth=1, hidden_size=64, intermediate_size=128, num_heads=2, out_hidden_size=3584)
    try:
        cfg = Qwen2_5_VLConfig(text_config=text, vision_config=vis)
    except TypeError:
        cfg = Qwen2_5_VLConfig(vision_config=vis, **text)
    m = Qwen2_5_VLForConditionalGeneration(cfg).eval()
    with torch.no_grad():
        for n, p in m.named_parameters():
            if 'layernorm' in n or n.endswith('norm.weight'):
                p.copy_(1 + 0.2 * torch.randn_like(p))
            if n.endswith('proj.bias'):
                p.copy_(0.3 * torch.randn_like(p))
    m = _bf16_weights(m)
    ids = torch.randint(0, 390, (1, 162))
    enc = Qwen25TextEncoder(m.state_dict(), num_layers=1, num_heads=28, num_kv_heads=4)
    if hasattr(m.config, 'text_config'):
        m.config.text_config._attn_implementation = 'eager'
    _layer_parity('qwen2.5-7b 1 layer S=162', m, lambda mod: (mod(input_ids=ids.cuda(), output_hidden_states=True).hidden_states[-1][0],),
                  lambda: (enc(ids)[0],))
