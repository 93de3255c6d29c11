"""ISA lint for the gfx950 kernels (no GPU needed): compile a .hip file to device
assembly and list, per kernel, the `s_waitcnt vmcnt(N)` values that sit inside
loop bodies.  A vmcnt(0) in a pipelined loop means the ring is not prefetching
(round 3: a branch around the ring loads of the C8 weight gradient made hipcc
merge the counters of both paths -- every step waited for the loads it had just
issued).  `--epilogue` also counts vmcnt(0) outside loops (a chain of dependent
loads: round 3's may-alias epilogue had 155 in one kernel).

    python tools/isa_lint.py ld_amd/csrc/conv_bf16.hip [--match wgrad] [--epilogue]

`--against OTHER.s` compares the file (a .hip source or an already compiled .s)
with another tree's assembly, kernel by kernel under the same mangled name: one
line each with identical / loops identical (same code from the entry to the end
of the last loop, branch labels renumbered) / different, and VGPRs (waves per
SIMD), SGPRs, LDS and scratch bytes of both.  Exit status 1 when a kernel is
different, missing, or moves in scratch, LDS or waves per SIMD.
"""
import argparse
import os
import re
import subprocess
import sys
import tempfile

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def device_asm(src):
    out = tempfile.mktemp(suffix='.s')
    cmd = [os.environ.get('HIPCC', '/opt/rocm/bin/hipcc'), '-O3', '--offload-arch=gfx950',
           '-std=c++17', '-I' + os.path.join(REPO, 'include'),
           '-I' + os.path.join(REPO, 'ld_amd', 'csrc'), '--cuda-device-only', '-S', src,
           '-o', out]
    subprocess.run(cmd, check=True, stderr=subprocess.DEVNULL)
    text = open(out).read()
    os.remove(out)
    return text


def lint(text, match='', epilogue=False):
    lines = text.split('\n')
    starts = [(i, l.split(':')[0]) for i, l in enumerate(lines)
              if re.match(r'^_Z\w*kernel\w*:\s', l)]
    rows = []
    for n, (i, name) in enumerate(starts):
        if match and match not in name:
            continue
        end = starts[n + 1][0] if n + 1 < len(starts) else len(lines)
        inloop, hist, outside0 = False, {}, 0
        for l in lines[i:end]:
            if 'Loop Header' in l or 'in Loop' in l:
                inloop = True
            elif l.startswith('.LBB'):
                inloop = False
            m = re.search(r's_waitcnt vmcnt\((\d+)\)', l)
            if not m:
                continue
            if inloop:
                hist[int(m.group(1))] = hist.get(int(m.group(1)), 0) + 1
            elif int(m.group(1)) == 0:
                outside0 += 1
        short = re.sub(r'_ZN12_GLOBAL__N_1\d+', '', name)
        rows.append((short, hist, outside0))
    return rows


def kernels(text):
    """name -> (code to the end of the last loop, whole code, resources)"""
    out = {}
    for m in re.finditer(r'^(_Z\w*kernel\w*):\s(.*?)^\.Lfunc_end', text, re.M | re.S):
        code, last, inloop, labels = [], 0, False, {}
        for l in m.group(2).split('\n'):
            if l.startswith(('.LBB', '; %bb.')):  # a block starts (label / fall-through)
                inloop = 'Loop Header' in l or 'in Loop' in l
            l = l.split(';')[0].strip()
            if not l or l.startswith('.amdhsa') or l.startswith('.end_amdhsa'):
                continue
            code.append(re.sub(r'\.LBB\d+_\d+',
                               lambda x: labels.setdefault(x.group(0), f'L{len(labels)}'), l))
            last = len(code) if inloop else last
        res = [max(int(v) for v in re.findall(rf'\.amdhsa_{k} (\d+)', m.group(2)))
               for k in ('next_free_vgpr', 'next_free_sgpr', 'group_segment_fixed_size',
                         'private_segment_fixed_size')]
        out[m.group(1)] = (code[:last], code, res)
    return out


def against(new, old, match=''):
    bad = len(set(new) ^ set(old))
    for name in sorted(set(new) ^ set(old)):
        print(f'only in {"this" if name in new else "the other"} tree: {name}')
    for name in sorted(set(new) & set(old)):
        if match not in name:
            continue
        (nl, nc, nr), (ol, oc, orr) = new[name], old[name]
        verdict = 'identical' if nc == oc else 'loops identical' if nl == ol else 'different'
        waves = [512 // ((r[0] + 7) // 8 * 8) for r in (orr, nr)]
        moved = verdict == 'different' or nr[2:] != orr[2:] or waves[0] != waves[1]
        bad += bool(moved)
        print(f'{verdict:16s}vgpr {orr[0]}>{nr[0]} (waves {waves[0]}>{waves[1]}) sgpr {orr[1]}>'
              f'{nr[1]} lds {orr[2]}>{nr[2]} scratch {orr[3]}>{nr[3]}'
              f'{"  <-- CHECK" if moved else ""}  {name}')
    return bad


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('src')
    ap.add_argument('--match', default='')
    ap.add_argument('--epilogue', action='store_true')
    ap.add_argument('--against', metavar='OTHER.s')
    a = ap.parse_args()
    if a.against:
        text = open(a.src).read() if a.src.endswith('.s') else device_asm(a.src)
        sys.exit(1 if against(kernels(text), kernels(open(a.against).read()), a.match) else 0)
    bad = 0
    for name, hist, out0 in lint(device_asm(a.src), a.match, a.epilogue):
        flag = ''
        if hist.get(0, 0) and len(hist) <= 3:
            flag = '   <-- vmcnt(0) dominates the loop'
            bad += 1
        tail = f'  vmcnt(0) outside loops: {out0}' if a.epilogue else ''
        if hist or a.epilogue:
            print(f'{name[:78]:78s} {dict(sorted(hist.items()))}{tail}{flag}')
    sys.exit(1 if bad else 0)


if __name__ == '__main__':
    main()
