"""The ISA audit arcflow_amd/build.py runs after every build (arcflow_amd/isa_audit.py), on synthetic assembly and through the product's own rule table
(CPU): a compiler-generated instruction that names an asm-owned register, or scratch in a kernel that must not have any, must fail the build; the
kernel's own asm statements (between ASMSTART / ASMEND), hipcc's parking below an accumulator base and kernels without a rule must not."""
import pytest

from arcflow_amd.isa_audit import RULES, Rule, audit


def asm(*lines):
    return [';;#ASMSTART', *lines, ';;#ASMEND']


def kernel(name, body, scratch=0):
    """A kernel as hipcc prints it: the label, the code, then the descriptor in .rodata."""
    return '\n'.join([f'\t.globl\t{name}', f'{name}: ; @{name}', *('\t' + t for t in body), '.Lfunc_end0:', '\t.section\t.rodata,"a",@progbits',
                      f'\t.amdhsa_kernel {name}', f'\t\t.amdhsa_private_segment_fixed_size {scratch}', '\t.end_amdhsa_kernel', '\t.text', ''])


def write(tmp_path, kernels, extra=None, scratch=None):
    """kernels: name -> (body, scratch).  `extra` appends compiler-generated lines to the named kernels, `scratch` overrides their scratch size."""
    text = ''.join(kernel(name, body + (extra or {}).get(name, []), (scratch or {}).get(name, size)) for name, (body, size) in kernels.items())
    p = tmp_path / 'k.s'
    p.write_text(text)
    return str(p)


def v3(mi, nj, conv=0, persist=0):
    return f'_ZN3afx14gemm_kernel_v3ILi{mi}ELi{nj}ELb{conv}ELi{persist}EEEvNS_9GemmBatchE'


V3S = '_ZN3afx15gemm_kernel_v3sILi4ELi4ELb0ELi0EEEvNS_9GemmBatchE'
V3F8 = '_ZN3afx16gemm_kernel_v3f8ILi8ELi8ELb0EEEvNS_9GemmBatchE'
PLAIN = '_ZN3afx11gemm_kernelILi4ELi4EEEvNS_9GemmBatchE'       # no rule names it
V3_BODY = ['v_add_u32_e32 v1, v2, v3', *asm('v_mfma_f32_16x16x32_bf16 a[0:3], v[4:7], v[8:11], a[0:3]'), *asm('v_accvgpr_read_b32 v12, a17'),
           'buffer_store_dwordx4 v[12:15], v1, s[8:11], 0 offen']
GEMM = {v3(8, 8): (V3_BODY, 0), v3(8, 7): (V3_BODY, 0), v3(7, 8): (V3_BODY, 0), v3(9, 6): (V3_BODY, 0),
        v3(10, 6): (V3_BODY, 16), v3(8, 8, conv=1): (V3_BODY, 64), v3(8, 8, persist=1): (V3_BODY, 8),       # the zero-scratch rule is not asked of these
        V3S: (['v_accvgpr_write_b32 a3, v1', 'v_accvgpr_read_b32 v1, a31',                                      # hipcc parking below the base
               *asm('v_mfma_f32_16x16x32_bf16 a[32:35], v[4:7], v[8:11], a[32:35]')], 0),
        V3F8: (['v_add_u32_e32 v1, v2, v3', *asm('v_mfma_f32_16x16x128_f8f6f4 a[200:203], v[4:11], v[12:19], a[200:203]'),
                *asm('v_accvgpr_read_b32 v1, a200')], 0),
        PLAIN: (['v_accvgpr_read_b32 v1, a200', 'scratch_store_dword off, v1, off'], 128)}
GEMM_RULES = RULES['afx_gemm.hip']


def test_accumulator_audit_accepts_asm_owned_use_and_parking_below_the_base(tmp_path):
    audit(write(tmp_path, GEMM), GEMM_RULES)


@pytest.mark.parametrize('bad', ['\tv_accvgpr_read_b32 v9, a40\n', '\tscratch_store_dwordx4 off, a[36:39], off offset:16\n', '\tv_accvgpr_mov_b32 a32, a2\n'])
def test_accumulator_audit_rejects_compiler_generated_access(tmp_path, bad):
    bad = bad.strip()
    with pytest.raises(RuntimeError, match='asm-owned accumulator') as e:
        audit(write(tmp_path, GEMM, extra={V3S: [bad]}), GEMM_RULES)
    assert V3S in str(e.value) and '1 instructions' in str(e.value) and bad in str(e.value)
    with pytest.raises(RuntimeError, match='asm-owned accumulator'):       # base 0: nothing of the file is hipcc's
        audit(write(tmp_path, GEMM, extra={v3(8, 8): ['v_accvgpr_write_b32 a0, v5']}), GEMM_RULES)


def test_accumulator_audit_covers_the_fp8_kernel(tmp_path):
    with pytest.raises(RuntimeError, match='asm-owned accumulator') as e:
        audit(write(tmp_path, GEMM, extra={V3F8: ['v_accvgpr_read_b32 v1, a200']}), GEMM_RULES)
    assert V3F8 in str(e.value)


@pytest.mark.parametrize('name', [v3(8, 8), v3(10, 6), v3(8, 8, conv=1), V3F8])
def test_accumulator_base_is_chosen_by_the_suffix_of_the_kernel_name(tmp_path, name):
    """a31 is hipcc's in gemm_kernel_v3s<...> (base 32, GEMM parks there) and asm-owned in gemm_kernel_v3<...> and gemm_kernel_v3f8<...> (base 0)."""
    with pytest.raises(RuntimeError, match='asm-owned accumulator') as e:
        audit(write(tmp_path, GEMM, extra={name: ['v_accvgpr_read_b32 v1, a31']}), GEMM_RULES)
    assert name in str(e.value) and V3S not in str(e.value)


def test_accumulator_audit_notices_a_renamed_kernel(tmp_path):
    with pytest.raises(RuntimeError, match=r"gemm_kernel_v4I.* found no kernel: update RULES in arcflow_amd/isa_audit\.py"):
        audit(write(tmp_path, GEMM), GEMM_RULES + [Rule('gemm_kernel_v4I', acc_base=0)])
    gone = {k: v for k, v in GEMM.items() if k != v3(9, 6)}       # every rule of the product's table must find its kernel
    with pytest.raises(RuntimeError, match='gemm_kernel_v3ILi9ELi6ELb0ELi0E.* found no kernel'):
        audit(write(tmp_path, gone), GEMM_RULES)


@pytest.mark.parametrize('name', [v3(8, 8), v3(8, 7), v3(7, 8), v3(9, 6), V3S, V3F8])
def test_scratch_in_a_listed_kernel_is_rejected_with_its_size(tmp_path, name):
    with pytest.raises(RuntimeError, match='uses 16 bytes of scratch: a spill inside an inline-asm MFMA stream') as e:
        audit(write(tmp_path, GEMM, scratch={name: 16}), GEMM_RULES)
    assert name in str(e.value)
    audit(write(tmp_path, GEMM, scratch={name: 16}), GEMM_RULES, check_scratch=False)       # what a variant build asks for
    audit(write(tmp_path, GEMM, scratch={name: 0}), GEMM_RULES)


def test_every_violation_of_the_file_is_in_the_one_error(tmp_path):
    with pytest.raises(RuntimeError) as e:
        audit(write(tmp_path, GEMM, extra={v3(8, 7): ['v_accvgpr_read_b32 v1, a5'] * 25, V3F8: ['v_accvgpr_read_b32 v1, a7']}, scratch={V3S: 32}), GEMM_RULES)
    msg = str(e.value)
    assert 'k.s' in msg and v3(8, 7) in msg and '25 instructions' in msg and V3F8 in msg and 'uses 32 bytes of scratch' in msg and PLAIN not in msg
    assert msg.count('v_accvgpr_read_b32 v1, a5') == 20       # the first 20 lines of a kernel


def test_rules_that_disagree_on_one_kernel_are_an_error(tmp_path):
    with pytest.raises(RuntimeError, match='disagree'):
        audit(write(tmp_path, GEMM), GEMM_RULES + [Rule('gemm_kernel_v3sILi4E', acc_base=0)])


ATTN = '_ZN3afx2a319attention_v3_kernelEPKtlS2_lPt'
ATTN_BODY = ['v_add_u32_e32 v95, v1, v2', 'v_pk_mul_f32 v[94:95], v[2:3], v[4:5]', 'buffer_store_dword v95, v1, s[8:11], 0 offset:16']
OWNED = ['v_mov_b32_e32 v96, v1', 'v_pk_mul_f32 v[94:97], v[2:5], v[6:9]', 'ds_write_b32 v1, a3', 'v_accvgpr_read_b32 v1, a0', 'scratch_load_dword v1, off, off',
         'buffer_store_dword v1, v2, s[8:11], 0 offen']


def test_vgpr_limit_accepts_the_registers_below_it_and_everything_inside_asm(tmp_path):
    audit(write(tmp_path, {ATTN: (ATTN_BODY + asm(*OWNED), 0), PLAIN: (OWNED, 128)}), RULES['afx_attn3.hip'])


@pytest.mark.parametrize('bad', OWNED)
def test_vgpr_limit_rejects_compiler_generated_use_of_asm_owned_registers(tmp_path, bad):
    with pytest.raises(RuntimeError, match='asm-owned registers') as e:
        audit(write(tmp_path, {ATTN: (ATTN_BODY + asm(*OWNED), 0)}, extra={ATTN: [bad]}), RULES['afx_attn3.hip'])
    assert ATTN in str(e.value) and '1 instructions' in str(e.value) and f'{len(ATTN_BODY) + len(OWNED) + 5}: {bad}' in str(e.value)


BWD = {f'_ZN3afx2b3{len(k)}{k}EPKtlS2_lPt': (['v_add_u32_e32 v59, v1, v2', *asm('v_mov_b32_e32 v200, v60')], 0)
       for k in ('attn_bwd_dkv3_kernel', 'attn_bwd_dq3_kernel', 'attn_bwd_fused3_kernel')}


@pytest.mark.parametrize('name', list(BWD))
def test_vgpr_limit_covers_the_three_backward_kernels_at_60(tmp_path, name):
    audit(write(tmp_path, BWD), RULES['afx_attn_bwd3.hip'])
    with pytest.raises(RuntimeError, match='asm-owned registers') as e:
        audit(write(tmp_path, BWD, extra={name: ['v_mov_b32_e32 v60, v1']}), RULES['afx_attn_bwd3.hip'])
    assert name in str(e.value) and sum(k in str(e.value) for k in BWD) == 1
    with pytest.raises(RuntimeError, match='found no kernel'):
        audit(write(tmp_path, {k: v for k, v in BWD.items() if k != name}), RULES['afx_attn_bwd3.hip'])
