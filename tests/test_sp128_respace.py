"""Placement of the ratio stage in the rank-128 software-pipelined MU kernel (csrc/nmfmu_sp128.h, template parameter RB).

RB reciprocals of tile t+1 run in the MFMA gaps of phase B(t), in place on the S registers; what stays in phase A(t+1) is
spread by issue cost (reciprocal = 2 plain).  Mirrored here -- sp128_phase_b / sp128_phase_a and the walk of group() and of
the prologue -- and replayed per wave for 4, 8 and 12 tiles per workgroup (the last group alone, one looped group + the
last, two looped groups + the last):

* every S element of every tile gets exactly one reciprocal, one multiply, and every pair one pack, in that order;
* a reciprocal comes after the last GEMM1 MFMA into its S tile with at least two MFMAs (or the prologue's pads) between --
  the XDL write -> VALU read distance -- and is never consumed by the instruction right behind it;
* nothing of tile t's ratio stage touches S[t & 1] while a GEMM1 writes that buffer, X(t) is read after its counted wait and
  before the loads of X(t+2) overwrite it, the ratios of tile t are complete before GEMM2(t) and are not overwritten before
  its last MFMA;
* phase A carries at most two reciprocals and 24 cycles of VALU issue per gap, phase B at most two reciprocals per gap for
  the shipped RB, none in its first three gaps.

On the compiled shipped instance (the library's own flags): the per-gap reciprocal counts are the tables', no gap has more
than two, and no s_nop of hipcc's stands next to a ratio-stage instruction.  hipcc pads in front of an asm statement that
touches a register an earlier asm statement wrote unless one of its own instructions lies between the two; with the ratio
stage's own pads gone (117 per four-tile group at RB = 0) the MFMA chains take theirs, behind the counted waits: 40 per group
at RB = 48 (34 s_waitcnt -> MFMA, 6 MFMA -> s_add_u32 of an LDS-DMA piece) against 135 at RB = 0 -- more than the 18 such
seams of the RB = 0 schedule, which stood in the shadow of the ratio stage's pads.  The count is printed, not bounded.
"""
import os
import re
import shutil
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, 'pytorch-nmf_amd', 'csrc')
N1, N2, PF = 16, 16, 4
DIST = 24                                    # kSP128Dist


def _shipped_rb():
    src = open(os.path.join(CSRC, 'nmfmu_inst_sp128.hip')).read()
    return int(re.search(r'#define NMFMU_SP128_RB (\d+)', src).group(1))


def _b_busy(gap):
    return gap % 2 == 0 and (gap // 2 < 4 or gap // 2 >= 8)


def _phase_b(rb):
    """sp128_phase_b: moved reciprocals per gap of phase B."""
    cnt, left = [0] * 32, rb
    for p in range(7):
        for g in range(3, 32):
            cls = 0 if g & 1 else (2 if _b_busy(g) else 1)
            if left > 0 and cls == (0 if p == 6 else p >> 1):
                cnt[g] += 1
                left -= 1
    assert left == 0
    first = [0]
    for g in range(32):
        first.append(first[-1] + cnt[g])
    return first


def _phase_a(rb):
    """sp128_phase_a: (first[33], op[]) with op = kind * 64 + index."""
    pos_r, pos_m = [-1000] * 64, [0] * 64
    nr, nm, nc, op, first = rb, 0, 0, [], []
    cost_left = 2 * (64 - rb) + 64 + 32
    for g in range(32):
        first.append(len(op))
        flush = g == 31
        budget = (cost_left + (32 - g) - 1) // (32 - g)
        used = 0
        c = 0
        while c < 2 and nr < 64 and used + 2 <= budget:
            pos_r[nr] = len(op)
            op.append(nr)
            nr += 1
            used += 2
            c += 1
        while nm < 64 and nm < nr and (flush or (used < budget and len(op) - pos_r[nm] >= DIST)):
            pos_m[nm] = len(op)
            op.append(64 + nm)
            nm += 1
            used += 1
        while nc < 32 and 2 * nc + 1 < nm and (flush or (used < budget and len(op) - pos_m[2 * nc + 1] >= DIST)):
            op.append(128 + nc)
            nc += 1
            used += 1
        cost_left -= used
    first.append(len(op))
    return first, op


def _entry(n, last):
    it, l = divmod(n, N1 + N2)
    if last and it == 3:
        return (3, False, l)
    return (it, l < N1, l if l < N1 else l - N1)


def _unit(u):
    """unit -> (tt, og): the S tile its four elements live in."""
    return u >> 3, (u >> 2) & 1


def _replay(rb, nt):
    """The instruction stream of one wave over nt tiles as a list of events, in issue order."""
    fb = _phase_b(rb)
    fa, opa = _phase_a(rb)
    ev = []

    def table(tile, lo, hi):
        for code in opa[lo:hi]:
            kind, i = code >> 6, code & 63
            ev.append((('rcp', 'mul', 'pack')[kind], tile, i))

    for k in range(N1):                                   # prologue: GEMM1(0)
        ev.append(('g1', 0, k, 0))
        ev.append(('g1', 0, k, 1))
    ev.append(('pads',))                                  # s_nop 15; s_nop 7
    for x in range(rb):
        ev.append(('rcp', 0, x))
    for i0 in range(0, nt, 4):
        last = i0 + 4 >= nt
        length = 3 * (N1 + N2) + (N2 if last else N1 + N2)
        for n in range(length):
            it, g1, k = _entry(n, last)
            final = last and it == 3
            t = i0 + it
            if final and k == 0:
                table(t, 0, len(opa))                     # the last tile's un-hidden ratio stage
            if g1:
                ev.append(('g1', t + 1, k, 0))
                table(t, fa[2 * k], fa[2 * k + 1])
                ev.append(('g1', t + 1, k, 1))
                table(t, fa[2 * k + 1], fa[2 * k + 2])
                if k == N1 - 1:
                    ev.append(('barrier', t))
            else:
                ev.append(('g2', t, k, 0))
                if not final:
                    if k >= 8:
                        ev.append(('xload', t + 2))
                    for x in range(fb[2 * k], fb[2 * k + 1]):
                        ev.append(('rcp', t + 1, x))
                ev.append(('g2', t, k, 1))
                if not final:
                    for x in range(fb[2 * k + 1], fb[2 * k + 2]):
                        ev.append(('rcp', t + 1, x))
                    if k == N2 - 1:
                        ev.append(('wait_x', t + 1))
    return ev


@pytest.mark.parametrize('rb', [16, 32, 48, 64])
@pytest.mark.parametrize('nt', [4, 8, 12])
def test_replay_of_the_stream_tables(rb, nt):
    ev = _replay(rb, nt)
    at = {}
    for p, e in enumerate(ev):
        at.setdefault(e, []).append(p)
    mfma_pos = [p for p, e in enumerate(ev) if e[0] in ('g1', 'g2')]
    for t in range(nt):
        first_g2 = at[('g2', t, 0, 0)][0]
        last_g2 = at[('g2', t, N2 - 1, 1)][0]
        ratio = []
        for x in range(64):
            tt, og = _unit(x >> 2)
            assert len(at[('rcp', t, x)]) == 1 and len(at[('mul', t, x)]) == 1, (t, x)
            r, m = at[('rcp', t, x)][0], at[('mul', t, x)][0]
            # the last GEMM1 MFMA into S[t & 1][og][tt]: rank step 7 = entry 14 + tt
            w = at[('g1', t, 14 + tt, og)][0]
            between = sum(1 for q in mfma_pos if w < q < r)
            assert w < r and (between >= 2 or ('pads',) in ev[w:r]), (t, x, w, r)
            assert m >= r + 2, (t, x)                    # never consumed by the instruction right behind it
            ratio += [r, m]
        for y in range(32):
            assert len(at[('pack', t, y)]) == 1
            c = at[('pack', t, y)][0]
            assert c > at[('mul', t, 2 * y)][0] and c > at[('mul', t, 2 * y + 1)][0]
            assert c < first_g2                          # the ratios are complete before GEMM2(t) ...
            if t > 0:
                assert c > at[('g2', t - 1, N2 - 1, 1)][0]   # ... and not overwritten before GEMM2(t - 1) has read them
            ratio.append(c)
        # S[t & 1] is written by GEMM1(t) (done: checked above) and next by GEMM1(t + 2)
        if t + 2 < nt:
            assert max(ratio) < at[('g1', t + 2, 0, 0)][0], t
        # X(t): landed (prologue, or the counted wait that ends phase B(t - 1)), overwritten by the loads of X(t + 2) in B(t)
        muls = [at[('mul', t, x)][0] for x in range(64)]
        if t >= 2:
            assert min(muls) > at[('wait_x', t)][0]
        if ('xload', t + 2) in at:
            assert max(muls) < at[('xload', t + 2)][0]
        assert last_g2 > first_g2
    # the last tile's phase B issues no reciprocal; nothing is issued for a tile that does not exist
    assert all(e[1] < nt for e in ev if e[0] in ('rcp', 'mul', 'pack'))
    tail = at[('g2', nt - 1, 0, 0)][0]
    assert not any(e[0] == 'rcp' for e in ev[tail:])


@pytest.mark.parametrize('rb', [16, 32, 48, 64])
def test_cost_per_gap(rb):
    """Phase A: whole ratio stage minus the moved reciprocals, at most two reciprocals and six cost units (24 cycles of VALU
    issue at 4 cycles per plain instruction, 8 per reciprocal) per gap, consumers DIST instructions behind their producers
    everywhere but in the last gap, which takes what is left (packs).  Phase B: RB reciprocals, none in the first three
    gaps, the gaps without a load filled first."""
    first, op = _phase_a(rb)
    assert sorted(op) == sorted(list(range(rb, 64)) + list(range(64, 128)) + list(range(128, 160)))
    pos = {c: p for p, c in enumerate(op)}
    for g in range(32):
        ops = op[first[g]:first[g + 1]]
        nr = sum(1 for c in ops if c < 64)
        assert nr <= 2
        if g < 31 or rb >= 32:
            assert 2 * nr + (len(ops) - nr) <= 6, (rb, g, ops)
    for x in range(64):
        if x >= rb:
            assert pos[64 + x] - pos[x] >= (DIST if pos[64 + x] < first[31] else 2)
    for y in range(32):
        late = pos[128 + y] >= first[31]
        assert pos[128 + y] - max(pos[64 + 2 * y], pos[64 + 2 * y + 1]) >= (1 if late else DIST)
    fb = _phase_b(rb)
    cnt = [fb[g + 1] - fb[g] for g in range(32)]
    assert sum(cnt) == rb and cnt[:3] == [0, 0, 0]
    assert max(cnt) <= (2 if rb <= 48 else 3)
    free = [c for g, c in enumerate(cnt) if g >= 3 and not _b_busy(g)]
    busy = [c for g, c in enumerate(cnt) if g >= 3 and _b_busy(g)]
    assert not any(busy) or min(free) >= 2               # a gap with a load only after every other gap holds two


def _loop_stream(path):
    """(op, is_asm) of every instruction in the kernel's MFMA loop (the walk of tools/asm_audit.py, order kept)."""
    s = open(path).read()
    fn = [f for f in re.split(r'\n(?=_ZN5nmfmu\w+:)', s)[1:] if 'sp128' in f.split(':')[0]]
    assert len(fn) == 1
    hdr = lambda line, m: (('.L' + re.search(r'Header=(BB\d+_\d+)', line).group(1)) if 'Header=' in line
                           else (m.group(1) if 'Loop Header' in line else None))
    hdrs, cur = set(), None
    for line in fn[0].split('\n'):
        m = re.match(r'(\.LBB\d+_\d+):', line.strip())
        if m:
            cur = hdr(line, m)
        elif cur and 'v_mfma' in line:
            hdrs.add(cur)
    cur, in_asm, out = None, False, []
    for line in fn[0].split('\n'):
        t = line.strip()
        m = re.match(r'(\.LBB\d+_\d+):', t)
        if m:
            cur = hdr(line, m)
        elif t.startswith(';;#ASMSTART'):
            in_asm = True
        elif t.startswith(';;#ASMEND'):
            in_asm = False
        elif t and not t.startswith(';') and not t.startswith('.') and cur in hdrs:
            out.append((t.split()[0], in_asm))
    return out


def test_compiled_shipped_instance(tmp_path):
    hipcc = shutil.which('hipcc') or '/opt/rocm/bin/hipcc'
    if not os.path.exists(hipcc):
        pytest.skip('hipcc not available')
    rb = _shipped_rb()
    assert rb in (0, 16, 32, 48, 64)
    if rb == 0:
        pytest.skip('the shipped instance is the RB = 0 schedule: nothing re-spaced')
    flags = ['--offload-arch=gfx950', '-O3', '-std=c++17', '-fPIC', '-fno-slp-vectorize', '-Wno-inline-asm']
    r = subprocess.run([hipcc] + flags + ['-S', '--cuda-device-only', os.path.join(CSRC, 'nmfmu_inst_sp128.hip'), '-o',
                                          str(tmp_path / 'x.s')], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-2000:]
    stream = _loop_stream(str(tmp_path / 'x.s'))
    # reciprocals per MFMA gap: the loop body is one group of four tiles = 4 x (phase A, phase B); gap g follows MFMA g
    gaps, n, seen = [], 0, False
    for op, _ in stream:
        if op.startswith('v_mfma'):
            if seen:
                gaps.append(n)
            seen, n = True, 0
        elif op == 'v_rcp_f32':
            n += 1
    gaps.append(n)
    assert len(gaps) == 4 * 64 and max(gaps) <= 2, max(gaps)
    fa, opa = _phase_a(rb)
    fb = _phase_b(rb)
    want_a = [sum(1 for c in opa[fa[g]:fa[g + 1]] if c < 64) for g in range(32)]
    want_b = [fb[g + 1] - fb[g] for g in range(32)]
    assert gaps == (want_a + want_b) * 4
    # hipcc's pads: none next to a ratio-stage instruction
    ratio = {'v_rcp_f32', 'v_fma_mix_f32', 'v_cvt_pk_f16_f32'}
    pads = [i for i, (op, a) in enumerate(stream) if op == 's_nop' and not a]
    where = {}
    for i in pads:
        key = (stream[i - 1][0], stream[i + 1][0])
        where[key] = where.get(key, 0) + 1
    print(f'RB = {rb}: {len(pads)} s_nop of hipcc per four-tile group: {where}')
    assert not any(k[0] in ratio or k[1] in ratio for k in where), where
