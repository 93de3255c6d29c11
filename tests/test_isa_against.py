"""`tools/isa_lint.py --against`: the per-kernel comparison of two trees' device
assembly, on hand-written assembly text (no compiler, no GPU)."""
import os
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(REPO, 'tools'))


def _kernel(name, n, body, tail, vgpr=40, lds=1024, scratch=0):
    """One kernel as hipcc prints it: entry block, one loop, an epilogue."""
    return f"""
{name}:                                   ; @{name}
; %bb.0:
\ts_load_dword s4, s[0:1], 0x10
.LBB{n}_1:                                ; =>This Inner Loop Header: Depth=1
{body}
\ts_cbranch_scc1 .LBB{n}_1
; %bb.2:
{tail}
\ts_endpgm
\t.section\t.rodata,"a",@progbits
\t.amdhsa_kernel {name}
\t\t.amdhsa_group_segment_fixed_size {lds}
\t\t.amdhsa_private_segment_fixed_size {scratch}
\t\t.amdhsa_next_free_vgpr {vgpr}
\t\t.amdhsa_next_free_sgpr 16
\t.end_amdhsa_kernel
\t.text
.Lfunc_end{n}:
"""


LOOP = '\tv_add_f32_e32 v1, v1, v2\n\ts_add_i32 s5, s5, -1'
TAIL = '\tglobal_store_dword v0, v1, s[2:3]'


def test_against_verdicts_and_resources(capsys):
    import isa_lint
    old = isa_lint.kernels(_kernel('_Z8a_kernelv', 0, LOOP, TAIL) +
                           _kernel('_Z8b_kernelv', 1, LOOP, TAIL) +
                           _kernel('_Z8c_kernelv', 2, LOOP, TAIL) +
                           _kernel('_Z8d_kernelv', 3, LOOP, TAIL))
    # a: the same code under other label numbers; b: another epilogue; c: another
    # loop; d: same code, more registers (12 -> 6 waves per SIMD)
    new = isa_lint.kernels(_kernel('_Z8a_kernelv', 7, LOOP, TAIL) +
                           _kernel('_Z8b_kernelv', 1, LOOP, TAIL + '\n\ts_nop 0') +
                           _kernel('_Z8c_kernelv', 2, LOOP + '\n\ts_nop 0', TAIL) +
                           _kernel('_Z8d_kernelv', 3, LOOP, TAIL, vgpr=73))
    assert set(new) == set(old) and len(new) == 4
    assert new['_Z8a_kernelv'][2] == [40, 16, 1024, 0]
    bad = isa_lint.against(new, old)
    rows = {l.split()[-1]: l for l in capsys.readouterr().out.splitlines()}
    assert rows['_Z8a_kernelv'].startswith('identical') and 'CHECK' not in rows['_Z8a_kernelv']
    assert rows['_Z8b_kernelv'].startswith('loops identical')
    assert 'CHECK' not in rows['_Z8b_kernelv']
    assert rows['_Z8c_kernelv'].startswith('different') and 'CHECK' in rows['_Z8c_kernelv']
    assert 'vgpr 40>73 (waves 12>6)' in rows['_Z8d_kernelv'] and 'CHECK' in rows['_Z8d_kernelv']
    assert bad == 2


def test_against_reports_missing_kernels_and_moved_memory(capsys):
    import isa_lint
    old = isa_lint.kernels(_kernel('_Z8a_kernelv', 0, LOOP, TAIL) +
                           _kernel('_Z8b_kernelv', 1, LOOP, TAIL))
    new = isa_lint.kernels(_kernel('_Z8a_kernelv', 0, LOOP, TAIL, lds=2048, scratch=8))
    assert isa_lint.against(new, old) == 2
    out = capsys.readouterr().out
    assert 'only in the other tree: _Z8b_kernelv' in out
    assert 'lds 1024>2048 scratch 0>8  <-- CHECK' in out
