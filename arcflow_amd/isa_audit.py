"""The post-build ISA audit: what hipcc may not do in kernels that own registers by literal name inside inline assembly.

hipcc cannot see those registers, so arcflow_amd/build.py has it save the device assembly and checks every compiler-generated instruction (outside
ASMSTART / ASMEND) of the kernels in RULES after every build.  A new asm-owned kernel is registered by one Rule under its source file here, nowhere else.
"""
from __future__ import annotations

import re
from dataclasses import dataclass, field


@dataclass(frozen=True)
class Rule:
    """What is demanded of every kernel whose mangled name contains `match`.  A kernel matched by several rules obeys all of them."""
    match: str
    # v[vgpr_limit:255] and the whole accumulator file are asm-owned (tools/gen_attn3.py): no compiler-generated instruction names them, no
    # v_accvgpr_*, no scratch_* and no buffer_* ... offen (a wrong amdgpu_num_vgpr ceiling was exceeded once -- silent corruption -- and past the
    # right one hipcc spills into accumulator registers)
    vgpr_limit: int | None = None
    # the accumulator file is asm-owned from a<acc_base> up (literal names in every MFMA and epilogue read, afx_gemm.hip v3_mfma_lit / AccLit):
    # no compiler-generated instruction names a<k> with k >= acc_base; hipcc may park its own values below
    acc_base: int | None = None
    # private_segment_fixed_size must be 0: a spill may store an accumulator straight behind the inline-asm MFMA that is still writing it
    # (happened to gemm_kernel_v3f8 once its epilogue grew)
    no_scratch: bool = False


# source file -> rules.  The narrow gemm_kernel_v3 / v3s entries are the <MI, NJ, conv=false, persist=0> instances of the forward's hot loop and state
# all that is demanded of them; every other instance (conv, persist, <10,6>) has the broad entry only, which does not demand zero scratch.
RULES = {
    'afx_attn3.hip': [Rule('attention_v3_kernel', vgpr_limit=96)],
    'afx_attn_bwd3.hip': [Rule('attn_bwd_dkv3_kernel', vgpr_limit=60), Rule('attn_bwd_dq3_kernel', vgpr_limit=60), Rule('attn_bwd_fused3_kernel', vgpr_limit=60)],
    'afx_gemm.hip': [       # the I ends the template's name: gemm_kernel_v3I is no substring of gemm_kernel_v3sI / gemm_kernel_v3f8I
        Rule('gemm_kernel_v3I', acc_base=0),
        Rule('gemm_kernel_v3ILi8ELi8ELb0ELi0E', acc_base=0, no_scratch=True),
        Rule('gemm_kernel_v3ILi8ELi7ELb0ELi0E', acc_base=0, no_scratch=True),
        Rule('gemm_kernel_v3ILi7ELi8ELb0ELi0E', acc_base=0, no_scratch=True),
        Rule('gemm_kernel_v3ILi9ELi6ELb0ELi0E', acc_base=0, no_scratch=True),
        Rule('gemm_kernel_v3sI', acc_base=32),          # the 128x128 kernel: amdgpu_num_vgpr(160) leaves hipcc a[0:31]
        Rule('gemm_kernel_v3sILi4ELi4ELb0ELi0E', acc_base=32, no_scratch=True),
        Rule('gemm_kernel_v3f8I', acc_base=0, no_scratch=True),
    ],
}


@dataclass
class Kernel:
    name: str                                   # mangled
    scratch: int | None = None                  # private_segment_fixed_size of its descriptor, None without one
    code: list = field(default_factory=list)    # (line number, text) of the compiler-generated instructions


def kernels(asm_path: str) -> list:
    """One pass over a saved .s: every function of the file with its scratch size and the instruction lines hipcc generated for it -- the lines
    outside ASMSTART / ASMEND that are not comments, directives or labels."""
    found = {}
    cur = None
    in_asm = False
    with open(asm_path) as f:
        for n, line in enumerate(f, 1):
            t = line.strip()
            head = t.split(';')[0].strip()          # "_ZN3afx...E:      ; @_ZN3afx..."
            if head.endswith(':') and not head.startswith('.L'):
                cur = found.setdefault(head[:-1], Kernel(head[:-1]))
            elif head.startswith('.amdhsa_kernel '):        # the descriptor follows the code, in .rodata
                cur = found.setdefault(head.split()[1], Kernel(head.split()[1]))
            elif head.startswith('.amdhsa_private_segment_fixed_size ') and cur:
                cur.scratch = int(head.split()[1])
            elif 'ASMSTART' in t:
                in_asm = True
            elif 'ASMEND' in t:
                in_asm = False
            elif cur and not in_asm and t and t[0] not in ';.':
                cur.code.append((n, t))
    return list(found.values())


_REG = re.compile(r'\b([av])(\d+)\b|\b([av])\[\d+:(\d+)\]')


def _touches_owned(t: str, limit: int | None, base: int | None) -> bool:
    """Does the compiler-generated instruction `t` break vgpr_limit=limit or acc_base=base (None: not demanded)?"""
    regs = [(m.group(1) or m.group(3), int(m.group(2) or m.group(4))) for m in _REG.finditer(t.split(';')[0])]       # (file, highest index) of each operand
    if limit is not None and (t.startswith(('v_accvgpr', 'scratch_')) or t.startswith('buffer_') and 'offen' in t or any(f == 'a' or k >= limit for f, k in regs)):
        return True
    return base is not None and any(f == 'a' and k >= base for f, k in regs)


def audit(asm_path: str, rules, check_scratch: bool = True) -> None:
    """Apply `rules` to the kernels of a saved .s; raises one RuntimeError that lists every violation of the file."""
    errors = []
    matched = set()
    for k in kernels(asm_path):
        mine = [r for r in rules if r.match in k.name]
        matched.update(mine)
        limits = {r.vgpr_limit for r in mine} - {None}
        bases = {r.acc_base for r in mine} - {None}
        if len(limits) > 1 or len(bases) > 1:       # a broad and a narrow rule on one kernel must say the same
            errors.append(f'kernel {k.name}: its rules disagree on a limit or a base: {mine}')
            continue
        bad = [f'{n}: {t}' for n, t in k.code if _touches_owned(t, min(limits, default=None), min(bases, default=None))]
        if bad:
            what = 'asm-owned registers / spills' if limits else 'the asm-owned accumulator registers'
            errors.append(f'kernel {k.name}: compiler-generated code touches {what} ({len(bad)} instructions):\n' + '\n'.join(bad[:20]))
        if check_scratch and any(r.no_scratch for r in mine) and k.scratch != 0:
            errors.append(f'kernel {k.name} uses {"?" if k.scratch is None else k.scratch} bytes of scratch: a spill inside an inline-asm MFMA stream '
                          f'is not hazard-checked by hipcc -- reduce its register pressure')
    # a renamed kernel or a changed template signature would otherwise drop out of the audit silently
    errors += [f'{r} found no kernel: update RULES in arcflow_amd/isa_audit.py' for r in rules if r not in matched]
    if errors:
        raise RuntimeError(f'{asm_path}: the ISA audit failed:\n' + '\n'.join(errors))
