"""Index algebra of the software-pipelined MU kernel with 64 owner rows per wave (csrc/nmfmu_sp128.h), mirrored on the CPU.

A workgroup is four waves on a 256-row tile; wave w owns the rows of two 32-row groups og = 0 / 1 (the ping-pong kernel's
waves 2 w and 2 w + 1), so one panel operand read feeds the MFMAs of both groups.  Checked here, with integer-tagged data
and the documented MFMA / transposing-read lane maps of tests/test_layout_emulation.py:

* owner fragments, S tiles and accumulators of a 64-row wave land where the ratio stage, GEMM2 and the epilogues expect them;
* the X fragment order per lane (256-row tiles, one 4 KiB piece per 32 owner rows);
* the operand stream tables of a four-tile group and their counted LDS waits;
* the ring-slot schedule: no slot is overwritten before its last reader, every first reader comes after the landing barrier;
* the epilogue's row -> lane map covers every (row, rank) exactly once;
* the compiled instance's resource report: no scratch, at most 256 + 256 registers, nothing of hipcc's own inside the loop
  but scalar address arithmetic and wait-state padding.
"""
import os
import re
import sys

import numpy as np
import pytest

from test_layout_emulation import _tr_read, mfma_32x32x16, p1_offset, p1_swz, xp_index

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
R_PAD, ROWB, IMG = 128, 256, 64 * 256
KS, RT = R_PAD // 16, R_PAD // 32
N1, N2, PF, NSLOT = 16, 16, 4, 4


def _addresses(lane):
    """ga[kk], gb[2 m2 + h][rt] of nmfmu_sp128.h (the algebra of nmfmu_sp2.h)."""
    j, hl = lane & 31, lane >> 5
    row0 = 32 * ((j >> 2) & 1) + (j & 3) + 4 * (j >> 3)
    sw0 = p1_swz(row0, R_PAD)
    ga = [row0 * ROWB + (((2 * v + hl) ^ sw0) << 4) for v in range(KS)]
    grp, s16 = lane >> 4, lane & 15
    cslot, lr = 2 * (grp & 1) + ((s16 & 3) >> 1), (s16 >> 2) & 3
    gb = [[(32 * (grp >> 1) + (s16 >> 2)) * ROWB + (((cslot ^ c) | ((lr ^ p) << 2)) << 4) + 8 * (s16 & 1) for p in range(RT)]
          for c in range(4)]
    return ga, gb


@pytest.mark.parametrize('wave', range(4))
def test_one_tile_of_a_64_row_wave(wave):
    """GEMM1, the ratio stage's pairing of S with the lane's X words, GEMM2 and the accumulator -> (row, rank) map of one wave
    over one tile in ring slot 2, on small integers (exact in float64): every element of S = owner panel^T, of the X pairing and
    of num = G panel must come out where the kernel reads it."""
    rng = np.random.default_rng(wave)
    owner = rng.integers(0, 4, size=(256, R_PAD)).astype(np.float64)
    panel = rng.integers(0, 4, size=(64, R_PAD)).astype(np.float64)
    slot = 2
    lds = np.zeros(NSLOT * IMG // 2)                       # the ring, in 16-bit elements
    for row in range(64):
        for r in range(R_PAD):
            lds[slot * IMG // 2 + p1_offset(row, r, R_PAD)] = panel[row, r]
    oimg = np.zeros(256 * R_PAD)                           # the owner's row-major image in HBM
    for row in range(256):
        for r in range(R_PAD):
            oimg[p1_offset(row, r, R_PAD)] = owner[row, r]
    addr = [_addresses(lane) for lane in range(64)]
    acc_rows = set()
    for og in range(2):
        # owner fragments q[og][kk]: row m0, rank slice 16 kk + 8 hl .. +7
        q = np.zeros((KS, 64, 8))
        for lane in range(64):
            j, hl = lane & 31, lane >> 5
            m0 = (2 * wave + og) * 32 + j
            sw = p1_swz(m0 & 63, R_PAD) << 4
            for kk in range(KS):
                byte = m0 * ROWB + ((kk * 32 + hl * 16) ^ sw)
                q[kk, lane] = oimg[byte // 2: byte // 2 + 8]
                assert list(q[kk, lane]) == list(owner[m0, 16 * kk + 8 * hl: 16 * kk + 8 * hl + 8])
        # GEMM1: entry k = (tt = k & 1, kk = k >> 1), one ds_read_b128 at ga[kk] + 16 tt ROWB + slot IMG
        S = np.zeros((2, 64, 16))
        for k in range(N1):
            tt, kk = k & 1, k >> 1
            a = np.zeros((64, 8))
            for lane in range(64):
                byte = addr[lane][0][kk] + tt * 16 * ROWB + slot * IMG
                assert byte % 16 == 0 and tt * 16 * ROWB + slot * IMG < 65536
                a[lane] = lds[byte // 2: byte // 2 + 8]
            S[tt] = mfma_32x32x16(a, q[kk], S[tt])
        want = owner @ panel.T                              # [256 owner rows][64 panel rows]
        G = np.zeros((2, 64, 16))                           # the "ratio" of element e: a tag of (owner row, column)
        for tt in range(2):
            for lane in range(64):
                j, hl = lane & 31, lane >> 5
                m0 = (2 * wave + og) * 32 + j
                for e in range(16):
                    kcol = 32 * hl + 16 * tt + e
                    assert S[tt, lane, e] == want[m0, kcol], (og, tt, lane, e)
                    # the X word the ratio stage pairs with S[tt][e]: chunk 2 tt + (e >> 3), word (e >> 1) & 3, half e & 1 of
                    # the lane's 32 elements of this group -- its place in the packed target (G = 2: 256-row tiles)
                    chunk, word, half = 2 * tt + (e >> 3), (e >> 1) & 3, e & 1
                    local = ((wave * 2 + og) * 4 + chunk) * 64 * 8 + lane * 8 + 2 * word + half
                    assert xp_index(m0, kcol, 1, False, G=2) == local
                    G[tt, lane, e] = (m0 * 64 + kcol) % 7
        # GEMM2: entry k = (rt = k % RT, (tt, m2) = k / RT): two transposing reads, A operand = ratios 8 m2 .. 8 m2 + 7 of S^T tile tt
        acc = np.zeros((RT, 64, 16))
        for k in range(N2):
            rt, c4 = k % RT, k // RT
            tt, m2 = c4 >> 1, c4 & 1
            o0 = (16 * tt + 8 * m2) * ROWB + slot * IMG
            assert o0 + 4 * ROWB < 65536
            lo = _tr_read(lds, [addr[lane][1][2 * m2][rt] + o0 for lane in range(64)])
            hi = _tr_read(lds, [addr[lane][1][2 * m2 + 1][rt] + o0 + 4 * ROWB for lane in range(64)])
            b = np.concatenate([lo, hi], axis=1)
            acc[rt] = mfma_32x32x16(G[tt][:, 8 * m2: 8 * m2 + 8], b, acc[rt])
        Gm = np.fromfunction(lambda m, kc: (m * 64 + kc) % 7, (256, 64))
        num = Gm @ panel                                    # [256][R_PAD]
        for rt in range(RT):
            for lane in range(64):
                j, hl = lane & 31, lane >> 5
                for e in range(16):
                    row = (2 * wave + og) * 32 + (e & 3) + 8 * (e >> 2) + 4 * hl
                    assert acc[rt, lane, e] == num[row, 32 * rt + j], (og, rt, lane, e)
                    acc_rows.add((row, 32 * rt + j))
    assert acc_rows == {(64 * wave + r, c) for r in range(64) for c in range(R_PAD)}


def test_x_fragment_order_covers_the_tile():
    """The eight 1 KiB loads of a wave (two bases 4 KiB apart, offsets 0 .. 3 KiB, 16 bytes per lane) read exactly the wave's
    8 KiB of the 32 KiB tile, every byte once, and all four waves the whole tile."""
    seen = set()
    for wave in range(4):
        for og in range(2):
            for qi in range(4):
                for lane in range(64):
                    byte = wave * 8192 + og * 4096 + qi * 1024 + lane * 16
                    assert qi * 1024 <= 4095                 # 13-bit signed instruction offset
                    for b in range(16):
                        assert byte + b not in seen
                        seen.add(byte + b)
    assert seen == set(range(256 * 64 * 2))


def _entry(n, last):
    it, l = divmod(n, N1 + N2)
    if last and it == 3:
        return (3, False, l)
    return (it, l < N1, l if l < N1 else l - N1)


def _group_len(last):
    return 3 * (N1 + N2) + (N2 if last else N1 + N2)


def test_stream_tables_of_a_four_tile_group():
    """sp_entry / sp_younger at N1 = N2 = 16 with TWO MFMAs per entry: the counted lgkmcnt in front of entry n's first MFMA
    equals the LDS read instructions issued after entry n's own (ring depth 4; one ds_read_b128 per GEMM1 entry, two
    ds_read_b64_tr_b16 per GEMM2 entry) and fits the 4-bit counter; every accumulator sees its MFMAs in the ping-pong kernel's
    order (rank steps ascending in GEMM1, (tt, m2) ascending in GEMM2); a group issues 64 MFMAs per tile."""
    for last in (False, True):
        length = _group_len(last)
        in_flight = []
        for n in range(length + PF):
            if n >= PF:
                m = n - PF
                own = 1 if _entry(m, last)[1] else 2
                younger = sum(1 if _entry(k, last)[1] else 2 for k in range(m + 1, min(m + PF, length)))
                assert len(in_flight) == own + younger and younger <= 15
                del in_flight[:own]
            if n < length:
                in_flight += [n] * (1 if _entry(n, last)[1] else 2)
        assert not in_flight
        g1_order, g2_order = {}, {}
        mfmas = 0
        for n in range(length):
            it, g1, k = _entry(n, last)
            for og in range(2):
                mfmas += 1
                if g1:
                    g1_order.setdefault((it, og, k & 1), []).append(k >> 1)
                else:
                    g2_order.setdefault((it, og, k % RT), []).append(k // RT)
        assert mfmas == 2 * length
        assert all(v == list(range(KS)) for v in g1_order.values())
        assert all(v == [0, 1, 2, 3] for v in g2_order.values())
        assert len(g1_order) == (3 if last else 4) * 4 and len(g2_order) == 4 * 2 * RT


def test_ring_slot_schedule():
    """Panel tile u lives in ring slot u & 3.  Between two barriers (the one that ends phase A(t) and the one that ends
    A(t+1)) a wave runs B(t) and A(t+1): call that epoch t (the prologue and A(0) are epoch -1).  Waves are at most one epoch
    apart, so two accesses of different waves are ordered exactly when their epochs differ.  Tile u is written by the LDS-DMA
    issued in B(u-3) (tiles 0 .. 2: in the prologue) and awaited in front of the barrier that ends A(u-2); it is read by
    GEMM1(u) (phase A(u-1), the first PF entries issued at the tail of B(u-2) or at the group's head) and by GEMM2(u) (phase
    B(u), the first entries issued at the tail of A(u)).  Replay of the issue points over three groups."""
    def epoch_of(i0, it, g1):               # the phase an entry's MFMA sits in
        return i0 + it - 1 if g1 else i0 + it

    nt = 12
    reads = {}
    for i0 in range(0, nt, 4):
        last = i0 + 4 >= nt
        length = _group_len(last)
        for n in range(length):
            it, g1, k = _entry(n, last)
            tile = i0 + it + 1 if g1 else i0 + it
            if n < PF:                       # issued at the head of the group: the start of A(i0)
                ep = i0 - 1
            else:
                pit, pg1, _ = _entry(n - PF, last)
                ep = epoch_of(i0, pit, pg1)
            reads.setdefault(tile, []).append(ep)
            slot_of_entry = (it + 1) & 3 if g1 else it & 3
            assert slot_of_entry == tile & 3
    assert sorted(reads) == list(range(nt))  # (tile 0's GEMM1 runs in the prologue, its GEMM2 in the loop)
    write = {u: (-2 if u < 3 else u - 3) for u in range(nt)}      # epoch of the DMA issue (prologue: before everything)
    landed = {u: (-1 if u < 3 else u - 2) for u in range(nt)}     # first epoch in which every wave's pieces are visible
    for u in range(nt):
        assert min(reads[u]) >= landed[u], (u, reads[u])
        assert write[u] < landed[u]
        if u + NSLOT < nt:
            assert max(reads[u]) < write[u + NSLOT], (u, reads[u])
    # X buffers: X(t) is read by the ratio stage in A(t) and refilled with X(t+2) in B(t), after it; awaited at the end of B(t+1)
    # vmcnt arithmetic: B(t) issues 4 panel pieces, THEN 8 X loads; "vmcnt(8)" at the end of A(t+1) leaves the X loads,
    # "vmcnt(12)" at the end of B(t+1) leaves B(t+1)'s own twelve
    issued = []
    for t in range(6):
        issued += [('p', t + 3)] * 4 + [('x', t + 2)] * 8          # B(t)
        left = issued[-8:]                                          # A(t+1): vmcnt(8)
        assert all(kind == 'x' for kind, _ in left) and ('p', t + 3) not in left
        nxt = [('p', t + 4)] * 4 + [('x', t + 3)] * 8               # B(t+1) ... vmcnt(12)
        assert ('x', t + 2) not in (issued + nxt)[-12:]


def test_epilogue_row_lane_map():
    """Fused-apply epilogue: group (wave, og) plays the ping-pong kernel's wave 2 w + og -- staging tile 2 w + og, rows
    (2 w + og) 32 + i (64 / SP) + lane / SP, ranks 8 (lane % SP) .. + 7.  Every (row, rank) of the 256-row block exactly once;
    the staging tiles tile the 128 KiB; the column-sum partials land in eight distinct rows of the reduction buffer."""
    SP = R_PAD // 8
    nch = 32 * SP // 64
    seen = set()
    tiles = set()
    for wave in range(4):
        for og in range(2):
            v = 2 * wave + og
            tiles.add(v * 32 * R_PAD * 4)
            for i in range(nch):
                for lane in range(64):
                    row = v * 32 + i * (64 // SP) + lane // SP
                    for k in range(8):
                        key = (row, (lane % SP) * 8 + k)
                        assert key not in seen
                        seen.add(key)
    assert seen == {(r, c) for r in range(256) for c in range(R_PAD)}
    assert tiles == {t * 16384 for t in range(8)} and 8 * 16384 == 2 * 4 * 32 * R_PAD * 4
    # slab epilogue: accumulator register e of lane (j, hl), group v, rank tile rt
    seen = set()
    for v in range(8):
        for rt in range(RT):
            for lane in range(64):
                for e in range(16):
                    key = (v * 32 + (e & 3) + 8 * (e >> 2) + 4 * (lane >> 5), rt * 32 + (lane & 31))
                    assert key not in seen
                    seen.add(key)
    assert len(seen) == 256 * R_PAD


def test_compiled_instance_fits_the_register_file(tmp_path):
    """The resource report of the compiled instance (the library's own flags): no scratch, at most 256 VGPRs and 256 AGPRs,
    one wave per SIMD; inside the tile loop hipcc adds nothing but scalar address arithmetic and its own wait-state padding
    (tools/asm_audit.py) -- never a vector / accumulator move, a wait, M0 or a memory access."""
    import shutil
    import subprocess
    hipcc = shutil.which('hipcc') or '/opt/rocm/bin/hipcc'
    if not os.path.exists(hipcc):
        pytest.skip('hipcc not available')
    src = os.path.join(ROOT, 'pytorch-nmf_amd', 'csrc', 'nmfmu_inst_sp128.hip')
    flags = ['--offload-arch=gfx950', '-O3', '-std=c++17', '-fPIC', '-fno-slp-vectorize', '-Wno-inline-asm']
    r = subprocess.run([hipcc] + flags + ['-Rpass-analysis=kernel-resource-usage', '-S', '--cuda-device-only', src, '-o',
                                          str(tmp_path / 'x.s')], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-2000:]
    blocks = [b for b in r.stderr.split('Function Name: ')[1:] if 'sp128_kernel' in b.split('\n')[0]]
    assert len(blocks) == 1
    get = lambda key: int(re.search(re.escape(key) + r': (\d+)', blocks[0]).group(1))
    assert get('ScratchSize [bytes/lane]') == 0
    assert get(' VGPRs') <= 256 and get('AGPRs') <= 256 and get(' VGPRs') + get('AGPRs') <= 512
    assert get('AGPRs') >= 192                              # accumulators and owner fragments live there
    sys.path.insert(0, os.path.join(ROOT, 'tools'))
    import asm_audit
    res = asm_audit.audit(str(tmp_path / 'x.s'), 'sp128', verbose=False)
    assert len(res) == 1
    for name, (asm_ops, comp, comp_lines) in res.items():
        assert asm_ops['v_mfma_f32_32x32x16_f16'] == 4 * 64
        assert asm_ops['ds_read_b128'] == 4 * 16 and asm_ops['ds_read_b64_tr_b16'] == 4 * 32
        assert asm_ops['global_load_lds_dwordx4'] == 4 * 4 and asm_ops['global_load_dwordx4'] == 4 * 8
        assert asm_ops['v_rcp_f32'] == 4 * 64 and asm_ops['v_fma_mix_f32'] == 4 * 64 and asm_ops['v_cvt_pk_f16_f32'] == 4 * 32
        assert set(comp) <= {'s_nop', 's_add_u32', 's_addc_u32', 's_add_i32', 's_lshl_b64', 's_min_i32', 's_ashr_i32', 's_mov_b64',
                             's_mov_b32', 's_cmp_lt_i32', 's_cbranch_scc1', 's_mul_i32', 's_mul_hi_u32', 's_sub_i32', 's_lshl_b32',
                             's_and_b32', 's_or_b32', 's_cselect_b32', 's_cmp_eq_u32', 's_branch'}, (name, sorted(comp))
        assert not any('m0' in l for l in comp_lines), name
