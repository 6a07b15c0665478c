"""Device-code comparison of two trees of pytorch-nmf_amd/csrc (a refactor against its parent): per kernel symbol the
resource numbers hipcc reports, the text of the MFMA loops and the instruction counts of everything else.
    python tools/isa_compare.py OLD_CSRC NEW_CSRC [--work DIR] [--units a,b,...] [--whole a,b,...] [--jobs N] [--out FILE]
Each unit is compiled with the Makefile's flags plus -Rpass-analysis=kernel-resource-usage -S --cuda-device-only (about a
minute per unit); DIR keeps the assembly (old/<unit>.s, new/<unit>.s), a unit whose .s is already there is not recompiled.
One line per kernel: SGPRs / VGPRs / AGPRs / scratch bytes / occupancy / LDS bytes old -> new, instruction count outside
the MFMA loops old -> new, whether every loop block that holds an MFMA is the same text (or at least the same sequence of
mnemonics), and the mnemonics whose counts differ outside them.  For units whose device code must not change at all (--whole, default the NMFD GEMM units) the whole
assembly is compared.  Loop blocks are compared with their branch-target numbers erased (they shift with the code around
the loop).  Exit status 1 when a resource number, a loop block or a --whole unit differs."""
import argparse
import os
import re
import shutil
import subprocess
import sys
from collections import Counter
from concurrent.futures import ThreadPoolExecutor

UNITS = ['nmfmu_inst_r32', 'nmfmu_inst_r64', 'nmfmu_inst_r128', 'nmfmu_inst_r256', 'nmfmu_inst_pp', 'nmfmu_inst_sp',
         'nmfmu_inst_sp2a', 'nmfmu_inst_sp2b', 'nmfmu_nmfd', 'nmfmu_nmfd_ws']
FLAGS = ['--offload-arch=gfx950', '-O3', '-std=c++17', '-fPIC', '-Wno-inline-asm', '-fno-slp-vectorize']   # csrc/Makefile
RES = [('SGPRs', r'TotalSGPRs: (\d+)'), ('VGPRs', r' VGPRs: (\d+)'), ('AGPRs', r'AGPRs: (\d+)'),
       ('scratch', r'ScratchSize \[bytes/lane\]: (\d+)'), ('occupancy', r'Occupancy \[waves/SIMD\]: (\d+)'),
       ('LDS', r'LDS Size \[bytes/block\]: (\d+)')]


def compile_unit(csrc, unit, outdir):
    s, err = os.path.join(outdir, unit + '.s'), os.path.join(outdir, unit + '.remarks')
    if os.path.exists(s) and os.path.exists(err):
        return
    hipcc = shutil.which('hipcc') or '/opt/rocm/bin/hipcc'
    r = subprocess.run([hipcc] + FLAGS + ['-Rpass-analysis=kernel-resource-usage', '-S', '--cuda-device-only',
                                          os.path.join(csrc, unit + '.hip'), '-o', s + '.tmp'], capture_output=True, text=True)
    if r.returncode:
        sys.exit('%s: %s' % (unit, r.stderr[-3000:]))
    open(err, 'w').write(r.stderr)
    os.replace(s + '.tmp', s)


def resources(remarks):
    out = {}
    for b in remarks.split('Function Name: ')[1:]:
        out[b.split()[0]] = tuple(int(re.search(p, b).group(1)) for _, p in RES)
    return out


def kernels(asm):
    """name -> (texts of the loop blocks that belong to a loop with an MFMA, mnemonic counts of all other blocks)"""
    out = {}
    for fn in re.split(r'\n(?=_ZN5nmfmu\w+:)', asm)[1:]:
        name = fn.split(':')[0]
        body = fn.split('.Lfunc_end')[0]
        blocks, cur = [[None, []]], None          # [loop header or None, instruction lines]
        for line in body.split('\n'):
            t = line.strip()
            m = re.match(r'(\.LBB\d+_\d+):', t)
            if m:
                h = re.search(r'Header=(BB\d+_\d+)', line)
                cur = ('.L' + h.group(1)) if h else (m.group(1) if 'Loop Header' in line else None)
                blocks.append([cur, []])
            elif t and not t.startswith(';') and not t.startswith('.'):
                blocks[-1][1].append(re.sub(r'\s+', ' ', t))
        mfma = {h for h, ls in blocks if h and any(l.startswith('v_mfma') for l in ls)}
        loops = ['\n'.join(ls) for h, ls in blocks if h in mfma]
        rest = Counter(l.split()[0] for h, ls in blocks if h not in mfma for l in ls)
        out[name] = (loops, rest)
    return out


def strip_labels(loops):
    # block numbers shift when code outside the loops changes: compare the instructions with branch targets erased
    return [re.sub(r'\.LBB\d+_\d+', '.LBB', l) for l in loops]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('old')
    ap.add_argument('new')
    ap.add_argument('--work', default='isa_compare_work')
    ap.add_argument('--units', default=','.join(UNITS))
    ap.add_argument('--whole', default='nmfmu_nmfd,nmfmu_nmfd_ws')
    ap.add_argument('--jobs', type=int, default=4)
    ap.add_argument('--out', default=None)
    a = ap.parse_args()
    units = a.units.split(',')
    for side in ('old', 'new'):
        os.makedirs(os.path.join(a.work, side), exist_ok=True)
    with ThreadPoolExecutor(a.jobs) as ex:
        list(ex.map(lambda j: compile_unit(*j), [(getattr(a, side), u, os.path.join(a.work, side)) for u in units for side in ('old', 'new')]))
    lines, bad = [], False
    for u in units:
        rd = lambda side, ext: open(os.path.join(a.work, side, u + ext)).read()
        asm_o, asm_n = rd('old', '.s'), rd('new', '.s')
        res_o, res_n = resources(rd('old', '.remarks')), resources(rd('new', '.remarks'))
        k_o, k_n = kernels(asm_o), kernels(asm_n)
        lines.append('== %s: %d kernels' % (u, len(k_n)))
        if u in a.whole.split(','):
            cuid = lambda t: re.sub(r'__hip_cuid_\w+', '__hip_cuid', t)   # (a hash of the source text)
            same = cuid(asm_o) == cuid(asm_n)
            bad |= not same
            lines.append('   whole device assembly identical: %s' % ('yes' if same else 'NO'))
        if set(k_o) != set(k_n):
            bad = True
            lines.append('   KERNEL SYMBOLS DIFFER: only old %s, only new %s' % (sorted(set(k_o) - set(k_n)), sorted(set(k_n) - set(k_o))))
        for name in sorted(set(k_o) & set(k_n)):
            (lo, ro), (ln, rn) = k_o[name], k_n[name]
            loops_same = strip_labels(lo) == strip_labels(ln)
            res_same = res_o[name] == res_n[name]
            ops = lambda loops: [[l.split()[0] for l in b.split('\n') if l] for b in loops]
            loops_txt = 'yes' if loops_same else ('NO (same mnemonic sequence, operands differ)' if ops(lo) == ops(ln) else 'NO')
            bad |= not (loops_same and res_same)
            diff = {m: (ro[m], rn[m]) for m in sorted(set(ro) | set(rn)) if ro[m] != rn[m]}
            lines.append('%s: %s%s | instructions outside MFMA loops %d -> %d | %d MFMA loop blocks identical: %s%s' % (
                name[9:], ' '.join('%s %d -> %d' % (n, o, w) for (n, _), o, w in zip(RES, res_o[name], res_n[name])),
                '' if res_same else '  RESOURCES DIFFER', sum(ro.values()), sum(rn.values()), len(ln), loops_txt,
                (' | counts that differ: ' + ', '.join('%s %d -> %d' % (m, o, w) for m, (o, w) in diff.items())) if diff else ''))
    text = '\n'.join(lines) + '\n'
    sys.stdout.write(text)
    if a.out:
        open(a.out, 'w').write(text)
    sys.exit(1 if bad else 0)


if __name__ == '__main__':
    main()
