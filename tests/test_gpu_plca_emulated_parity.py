"""PLCA / SIPLCA EM kernels per element against float64 emulations with derived bounds (tests/plca_emulation.py).

a. The small kernels of nmfmu_plca.hip through the C ABI on synthetic inputs (numerators with zeros and negative entries;
   NaN in every output buffer, in the scratch and in the padding of the inputs a kernel must not read; guard words behind f):
   nmfmu_plca_em (every r_pad, groups == 1, no rank padding, rows 1 / 31 / 32 / 33 / 300 / 9 590 = unrolled finalize loop plus
   tail, 1 and 3 slabs, rows_pad > rows, update 0 / 1, zgrad_out null / non-null), nmfmu_plca_normalize followed by
   nmfmu_plca_scale (alpha 1 / 1.001 / 1.02 / 0.99, the grid-stride loop above 4096 x 256 elements), nmfmu_plca_z, nmfmu_plca3
   in its three modes, and the argument errors (NMFMU_ERR_ARG, nothing launched).  Every element of f, the column sums, Z.grad,
   prior and z against ``plca_emulation``'s value within its bound; padded rank columns of the sums exactly 0; f bit-unchanged
   at update == 0; sums of a renormalised column / of z within ``unit_sum_bound`` / ``zsum_bound`` of 1.
b. One EM step on ``_PlcaEM`` per element, for the six cases of ``plca_emulation.DENSE_CASES`` x the seven trainable
   combinations, the three prior settings rotating (``dense_steps``), each step started from the case's start state (see
   ``plca_emulation.split_plane_sensitivity`` for why not from its predecessor's result) and emulated from the state read
   back from the device: images (plain: bit-exact the rounding of the masters; fWz / fHz: of fp32(f z), zero padding), numerators after
   nmfmu_mu_partial alone (slabs poisoned; every element, summed over the splits, against ``mu_emulation.half_step`` with the
   split panel, at mu_emulation.TOL), masters after em_step against ``plca_emulation.em_step`` on the device's own slabs
   within the derived bounds, column sums and sum(Z), the float64 oracle at the project's bars (1e-4 bf16x3, 2e-2 bf16), and
   divergence() against the float64 KL of the images within ``kl_loss``'s bound.
   kModeMU2 with fp16 operands is reachable from no model (PLCA refuses the fp16 modes): it is covered AT THE ABI ONLY,
   through FactorBuf / StepBuf with NMFMU_STAGE_DMA_SPLIT on operands of order 1, numerators at TOL['f16'].
c. One EM step on ``_ConvPlcaEM`` (SIPLCA / SIPLCA2 / SIPLCA3), both TORCHNMF_AMD_NMFD_H_ROWS settings: wm_s planes bit-exact
   the rounding of fp32(W Z); num_w (after nmfmu_slab_sum) and numh per element against tests/conv_emulation.py fed with the
   device's ratio planes, at mu_emulation.TOL; W, H, Z against the emulated update from the device's numerators within the
   derived bounds; the float64 oracle at 1e-4; an exact zero of W stays an exact zero (where W takes no prior).  Five shapes:
   the four of test_siplca_several_shift_axes_on_window_tables_against_oracle / (2, 70, 304) with T = 16, none of which splits
   the (G^T H) contraction, and (4, 6, 256) with T = 8, which does (w_ksplit 2); three (train, prior) settings each.

No element is excluded anywhere.  Every bound is derived (plca_emulation's docstring) or an existing project tolerance.

Measured on the MI355X (62 tests, 5 s), largest fraction of each bound (1 = at the bound; a single correctly rounded operation
reaches its half-ulp bound, so the elementwise figures sit just below 1 by construction):
a. plca_em: f 0.96, column sums 0.045, Z.grad 0.039.  normalize: y 0.99, sums 0.076; scale from the device's y 1.00, from the
   inputs 0.66; renormalised column sums 0.072 of ``unit_sum_bound``.  plca_z: prior 0.98, z 0.26, sum(z) 0.19.  plca3: f 0.92,
   sums 0.037 / 0.062, Z.grad 0.029, y 0.92, scale 0.97, unit sums 0.057.
b. images: no mismatching word.  Numerators: 7.4e-7 (bf16x3, TOL 4e-6), 3.0e-7 after the ambiguity allowance (bf16, TOL
   2.5e-6), no NaN left, none negative.  Masters W 0.12, H 0.11, Z 0.05; column sums 0.064, unit sums 0.077, sum(Z) 0.16; loss
   0.0027 of its bound (3.8e-7 relative).  Oracle: 3.8e-6 (bf16x3, bar 1e-4), 1.5e-2 (bf16, bar 2e-2).  kModeMU2 / fp16 at the
   ABI: 3.5e-7 (TOL 2.5e-6).
c. wm_s / wmt_s and every ratio word exact (ambiguous share at most 0.2 %); num_w 7.1e-7, numh 3.7e-7 (TOL 4e-6); W 0.068,
   H 0.066, Z 0.027 of their bounds; oracle 6.6e-5 (bar 1e-4).
The same file against a library that still formed the prior constant as fp32(alpha) - 1.f: every dense and every convolutive
case, every normalize / plca3 case with a prior and the Z cases above rank 1 fail -- y 783 times its bound at alpha = 1.001,
z 64, the masters of a dense step 6.7, of a convolutive step 5.1 (the only alpha = 1.001 steps inside their bounds: Z alone
at rank 33, 0.99, and rank 1, where z is 1 whatever is added).
"""
import ctypes
from types import SimpleNamespace

import numpy as np
import pytest
import torch

from conftest import record, rel_err
import mu_emulation as E
import plca_emulation as P
import test_gpu_emulated_parity as G

pytestmark = pytest.mark.gpu

NAN = float('nan')
GUARD = 64
SENTINEL = 12345.0


@pytest.fixture(scope='module')
def dev():
    assert torch.cuda.is_available(), 'needs the MI355X'
    return torch.device('cuda:0')


@pytest.fixture(scope='module')
def lib():
    from torchnmf_amd import _capi
    return _capi.load()


def _s():
    return torch.cuda.current_stream().cuda_stream


def _up(a, dev):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32)).to(dev)


def _guarded(f, dev):
    """f flattened, followed by GUARD sentinel words."""
    buf = torch.full((f.size + GUARD,), SENTINEL, dtype=torch.float32, device=dev)
    buf[:f.size] = _up(f, dev).reshape(-1)
    return buf


def _nan(n, dev):
    return torch.full((max(int(n), 1),), NAN, dtype=torch.float32, device=dev)


def _padded_vec(v, n, dev):
    """v followed by NaN up to n entries (a kernel may read the first len(v) only)."""
    out = _nan(n, dev)
    out[:len(v)] = _up(v, dev)
    return out


def _np(t):
    return t.detach().cpu().numpy()


def _guard_ok(buf, n):
    return bool((buf[n:] == SENTINEL).all())


# ---- a. the small kernels through the C ABI ----------------------------------------------------------------------------
@pytest.mark.parametrize('i', range(len(P.EM_CASES)), ids=lambda i: '{rows}x{rank}-s{nslab}-p{rows_pad}-u{update}-z{zgrad}'.format(**P.EM_CASES[i]))
def test_plca_em_kernel(dev, lib, i):
    c = P.EM_CASES[i]
    rows, rank, nslab, rows_pad = c['rows'], c['rank'], c['nslab'], c['rows_pad']
    r_pad = P.pad_rank(rank)
    assert lib.nmfmu_pad_rank(rank) == r_pad
    f, num, z = P.synthetic((rows, rank), 11 + i, nslab)
    assert (num.sum(0) < 0).any() and ((num == 0).all(0)).any() or rows * rank < 8
    full = np.full((nslab, rows_pad, r_pad), np.nan, dtype=np.float32)        # NaN wherever the kernel must not read
    full[:, :rows, :rank] = num
    fb, nb_, zb = _guarded(f, dev), _up(full, dev), _padded_vec(z, r_pad, dev)
    part = _nan(lib.nmfmu_plca_part_bytes(rows, r_pad) // 4, dev)
    cs, zg = _nan(r_pad, dev), _nan(r_pad, dev)
    e = lib.nmfmu_plca_em(fb.data_ptr(), rows, rank, r_pad, nb_.data_ptr(), nslab, rows_pad, zb.data_ptr(), c['update'],
                          part.data_ptr(), cs.data_ptr(), zg.data_ptr() if c['zgrad'] else None, _s())
    torch.cuda.synchronize()
    assert e == 0
    k = P.chain_rows(rows, r_pad)
    em = P.stage_em(f, P.read_slabs(full, nslab, rows, rows_pad, r_pad, rank), z, k)
    got_f = _np(fb[:rows * rank]).reshape(rows, rank)
    res = dict(cs=P.excess(_np(cs)[:rank], em['cs']))
    if c['update']:
        res['f'] = P.excess(got_f, em['x'])
    else:
        assert np.array_equal(got_f.view(np.uint32), f.view(np.uint32))
    assert _guard_ok(fb, rows * rank)
    assert np.all(_np(cs)[rank:] == 0.0)
    if c['zgrad']:
        res['zg'] = P.excess(_np(zg)[:rank], em['zg'])
        assert np.all(_np(zg)[rank:] == 0.0)
    else:
        assert bool(torch.isnan(zg).all())                                   # a null zgrad_out: nothing written anywhere else
    record('plca_emulated_parity', kernel='plca_em', case=c, chain=k, **res)
    print(c, res)
    assert all(v <= 1.0 for v in res.values()), res


@pytest.mark.parametrize('c', P.NORM_CASES, ids=lambda c: '{rows}x{rank}-a{alpha}'.format(**c))
def test_plca_normalize_and_scale_kernels(dev, lib, c):
    rows, rank, alpha = c['rows'], c['rank'], c['alpha']
    r_pad = P.pad_rank(rank)
    f, d = P.norm_problem(c)
    fb, db = _guarded(f, dev), _padded_vec(d, r_pad, dev)
    part = _nan(lib.nmfmu_plca_part_bytes(rows, r_pad) // 4, dev)
    cs = _nan(r_pad, dev)
    e = lib.nmfmu_plca_normalize(fb.data_ptr(), rows, rank, r_pad, db.data_ptr(), alpha, part.data_ptr(), cs.data_ptr(), _s())
    torch.cuda.synchronize()
    assert e == 0
    k = P.chain_rows(rows, r_pad)
    nm = P.stage_normalize(f, d, alpha, k)
    y_dev, cs_dev = _np(fb[:rows * rank]).reshape(rows, rank).copy(), _np(cs).copy()
    res = dict(y=P.excess(y_dev, nm['y']), cs=P.excess(cs_dev[:rank], nm['cs']))
    assert np.all(cs_dev[rank:] == 0.0) and _guard_ok(fb, rows * rank)
    if alpha != 1:
        assert y_dev.min() >= P.EPS
    e = lib.nmfmu_plca_scale(fb.data_ptr(), rows, rank, cs.data_ptr(), _s())
    torch.cuda.synchronize()
    assert e == 0
    out = _np(fb[:rows * rank]).reshape(rows, rank)
    res['scale'] = P.excess(out, P.stage_scale(y_dev, cs_dev[:rank]))               # from the device's own y and sums
    res['both'] = P.excess(out, P.stage_scale(nm['y'], nm['cs']))                   # from the inputs, bounds composed
    res['unit'] = float(np.abs(out.astype(np.float64).sum(0) - 1).max() / P.unit_sum_bound(k))
    assert _guard_ok(fb, rows * rank)
    record('plca_emulated_parity', kernel='plca_normalize+scale', case=c, chain=k, clamped=float((y_dev == np.float32(P.EPS)).mean()),
           grid=P.grid_scale(rows * rank), **res)
    print(c, res)
    assert all(v <= 1.0 for v in res.values()), res


@pytest.mark.parametrize('c', P.Z_CASES, ids=lambda c: 'r{rank}-a{alpha}'.format(**c))
def test_plca_z_kernel(dev, lib, c):
    rank, alpha = c['rank'], c['alpha']
    z, zg = P.z_problem(c)
    assert rank < 3 or ((zg <= 0).any() and (zg == 0).any())
    zb, gb, pb = _guarded(z, dev), _padded_vec(zg, 256, dev), _nan(256, dev)
    e = lib.nmfmu_plca_z(zb.data_ptr(), gb.data_ptr(), rank, alpha, pb.data_ptr(), _s())
    torch.cuda.synchronize()
    assert e == 0
    em = P.stage_z(z, zg, alpha)
    got = _np(zb[:rank])
    res = dict(prior=P.excess(_np(pb)[:rank], em['prior']), z=P.excess(got, em['z']),
               zsum=float(abs(got.astype(np.float64).sum() - 1) / em['zsum_bound']))
    assert _guard_ok(zb, rank) and bool(torch.isnan(pb[rank:]).all())
    record('plca_emulated_parity', kernel='plca_z', case=c, **res)
    print(c, res)
    assert all(v <= 1.0 for v in res.values()), res


def _plca3(lib, mode, f, outer, rank, inner, num, pitch, vec, alpha, update, part, cs, zg):
    return lib.nmfmu_plca3(mode, f.data_ptr(), outer, rank, inner, None if num is None else num.data_ptr(), pitch,
                           vec.data_ptr(), alpha, update, part.data_ptr(), cs.data_ptr(), None if zg is None else zg.data_ptr(), _s())


@pytest.mark.parametrize('i', range(len(P.PLCA3_CASES)), ids=lambda i: '{outer}x{rank}x{inner}-p{pitch}'.format(**P.PLCA3_CASES[i]))
def test_plca3_kernels(dev, lib, i):
    c = P.PLCA3_CASES[i]
    outer, rank, inner = c['outer'], c['rank'], c['inner']
    pitch = c['pitch'] or rank * inner
    alpha = P.ALPHAS[(i + 1) % 4]
    f, num, z = P.synthetic((outer, rank, inner), 31 + i)
    full = np.full((outer, pitch), np.nan, dtype=np.float32)
    full[:, :rank * inner] = num[0].reshape(outer, rank * inner)
    k = P.chain_plca3(outer, inner)
    n = f.size
    fb, nb_, zb = _guarded(f, dev), _up(full, dev), _up(z, dev)
    part = _nan(lib.nmfmu_plca3_part_bytes(rank) // 4, dev)
    cs, zg = _nan(rank, dev), _nan(rank, dev)
    em = P.stage_em(f, num[0], z, k)
    res = {}
    # mode 0, update 0 with zgrad_out: f untouched, both sums
    assert _plca3(lib, 0, fb, outer, rank, inner, nb_, pitch, zb, 1.0, 0, part, cs, zg) == 0
    torch.cuda.synchronize()
    assert np.array_equal(_np(fb[:n]).view(np.uint32), f.reshape(-1).view(np.uint32))
    res['cs0'], res['zg'] = P.excess(_np(cs), em['cs']), P.excess(_np(zg), em['zg'])
    # mode 0, update 1, null zgrad_out
    cs.fill_(NAN), zg.fill_(NAN), part.fill_(NAN)
    assert _plca3(lib, 0, fb, outer, rank, inner, nb_, pitch, zb, 1.0, 1, part, cs, None) == 0
    torch.cuda.synchronize()
    x_dev, cs_dev = _np(fb[:n]).reshape(f.shape).copy(), _np(cs).copy()
    res['f'], res['cs'] = P.excess(x_dev, em['x']), P.excess(cs_dev, em['cs'])
    assert bool(torch.isnan(zg).all()) and _guard_ok(fb, n)
    # mode 1: divide by a positive divider (the device's sums can hold zeros with synthetic numerators), prior alpha
    d = (np.abs(cs_dev) + np.float32(0.5)).astype(np.float32)
    db, cs2 = _up(d, dev), _nan(rank, dev)
    part.fill_(NAN)
    assert _plca3(lib, 1, fb, outer, rank, inner, None, 0, db, alpha, 1, part, cs2, None) == 0
    torch.cuda.synchronize()
    nm = P.stage_normalize(x_dev, d, alpha, k)
    y_dev, cs2_dev = _np(fb[:n]).reshape(f.shape).copy(), _np(cs2).copy()
    res['y'], res['cs2'] = P.excess(y_dev, nm['y']), P.excess(cs2_dev, nm['cs'])
    # mode 2
    c2 = (cs2_dev + np.float32(0.25)).astype(np.float32) if alpha == 1 else cs2_dev          # (a zero sum only without a prior)
    assert _plca3(lib, 2, fb, outer, rank, inner, None, 0, _up(c2, dev), 1.0, 1, part, cs2, None) == 0
    torch.cuda.synchronize()
    out = _np(fb[:n]).reshape(f.shape)
    res['scale'] = P.excess(out, P.stage_scale(y_dev, c2))
    if alpha != 1:
        res['unit'] = float(np.abs(out.astype(np.float64).sum((0, 2)) - 1).max() / P.unit_sum_bound(k))
    assert _guard_ok(fb, n)
    record('plca_emulated_parity', kernel='plca3', case=c, alpha=alpha, chain=k, **res)
    print(c, alpha, res)
    assert all(v <= 1.0 for v in res.values()), res


def test_argument_errors_launch_nothing(dev, lib):
    from torchnmf_amd import _capi
    f, num, z = P.synthetic((33, 5), 1)
    fb, nb_, zb = _guarded(f, dev), _up(np.zeros((1, 64, 32)), dev), _padded_vec(z, 32, dev)
    part, cs, zg = _nan(256, dev), _nan(256, dev), _nan(256, dev)
    P_ = lambda t: t.data_ptr()
    bad = [
        lib.nmfmu_plca_em(P_(fb), 33, 5, 64, P_(nb_), 1, 64, P_(zb), 1, P_(part), P_(cs), P_(zg), _s()),      # r_pad != pad_rank
        lib.nmfmu_plca_em(P_(fb), 33, 5, 32, P_(nb_), 1, 32, P_(zb), 1, P_(part), P_(cs), P_(zg), _s()),      # rows_pad < rows
        lib.nmfmu_plca_em(P_(fb), 33, 5, 32, P_(nb_), 0, 64, P_(zb), 1, P_(part), P_(cs), P_(zg), _s()),      # nslab < 1
        lib.nmfmu_plca_normalize(P_(fb), 33, 5, 64, P_(zb), 1.02, P_(part), P_(cs), _s()),                    # r_pad != pad_rank
        lib.nmfmu_plca_z(P_(zb), P_(zg), 257, 1.02, P_(cs), _s()),                                            # rank above 256
        lib.nmfmu_plca3(0, P_(fb), 3, 5, 11, P_(nb_), 54, P_(zb), 1.0, 1, P_(part), P_(cs), P_(zg), _s()),    # num_pitch < rank * inner
        lib.nmfmu_plca3(3, P_(fb), 3, 5, 11, P_(nb_), 55, P_(zb), 1.0, 1, P_(part), P_(cs), P_(zg), _s()),    # mode outside 0..2
        lib.nmfmu_plca3(-1, P_(fb), 3, 5, 11, P_(nb_), 55, P_(zb), 1.0, 1, P_(part), P_(cs), P_(zg), _s()),
    ]
    torch.cuda.synchronize()
    assert bad == [_capi.ERR_ARG] * len(bad), bad
    assert np.array_equal(_np(fb[:f.size]).view(np.uint32), f.reshape(-1).view(np.uint32)) and _guard_ok(fb, f.size)
    assert all(bool(torch.isnan(t).all()) for t in (part, cs, zg)) and bool(torch.isnan(zb[5:]).all())
    assert np.array_equal(_np(zb[:5]), z)


# ---- b. one dense EM step --------------------------------------------------------------------------------------------
def _shim(fb, master):
    """A FactorBuf's images with another master to hold them to (``_check_images`` reads f, rows, rank, rows_pad, p*_*)."""
    return SimpleNamespace(f=torch.from_numpy(np.ascontiguousarray(master, dtype=np.float32)), rows=fb.rows, rank=fb.rank,
                           rows_pad=fb.rows_pad, p1_hi=fb.p1_hi, p1_lo=fb.p1_lo, p2_hi=fb.p2_hi, p2_lo=fb.p2_lo)


def _img(fb, r_pad, prec, rows, R):
    hi, lo = G._read_images(fb, r_pad, prec)
    return hi[:rows, :R], (None if lo is None else lo[:rows, :R])


def _numerators(em, st, which, Vn, prec):
    """Every numerator element after nmfmu_mu_partial alone, summed over the splits, against the split-panel emulation."""
    R, r_pad = em.R, em.r_pad
    owner = st.owner
    scaled, plain = (em.fHz, em.fH) if which == 'w' else (em.fWz, em.fW)
    M, K = owner.rows, plain.rows
    st.slab_num.fill_(NAN)
    em.be.mu_partial(st)
    torch.cuda.synchronize()
    slabs = st.slab_num.view(st.nsplit, owner.rows_pad, r_pad)
    nan_left = int(torch.isnan(slabs[:, :M, :R]).sum())
    num = slabs.double().sum(0).cpu().numpy()[:M, :R]
    X = Vn.T if which == 'w' else Vn
    hs = E.half_step(X, None, None, 1.0, prec, A_img=_img(owner, r_pad, prec, M, R), B_img=_img(scaled, r_pad, prec, K, R),
                     B2_img=_img(plain, r_pad, prec, K, R))
    return dict(err=float(E.elem_err(num, hs['num'], hs['num_amb']).max()), raw=float(E.elem_err(num, hs['num']).max()),
                nan_left=nan_left, negative=int((num < 0).sum()))


def _slab_planes(st, R):
    return st.slab_num.view(st.nsplit, st.owner.rows_pad, st.r_pad)[:, :st.owner.rows, :R].double().cpu().numpy()


def _dense_em_step(em, Vn, prec, train, alphas):
    from oracle import mu_oracle as O
    R, r_pad = em.R, em.r_pad
    tW, tH, tZ = train
    aW, aH, aZ = alphas
    W0, H0, Z0 = _np(em.W).copy(), _np(em.H).copy(), _np(em.Z).copy()
    N, C = H0.shape[0], W0.shape[0]
    res = {}
    # images the step reads
    bad = {}
    for name, fb, master in (('fW', em.fW, W0), ('fWz', em.fWz, W0 * Z0[None, :]), ('fH', em.fH, H0), ('fHz', em.fHz, H0 * Z0[None, :])):
        bad[name] = G._check_images(_shim(fb, master), r_pad, prec, False)
    res['image_mismatch'] = sum(sum(b.values()) for b in bad.values())
    # loss of this state
    got = em.divergence()
    x = E.stored_target(Vn, prec)
    want, bound = P.kl_loss(x, _img(em.fH, r_pad, prec, N, R), _img(em.fWz, r_pad, prec, C, R),
                            r_pad * (3 if prec == 'bf16x3' else 1), em.fW.rows_pad // 64)
    res['loss'] = abs(got - want) / bound
    res['loss_rel'] = abs(got - want) / abs(want)
    # numerators
    res['num_w'] = _numerators(em, em.step_w, 'w', Vn, prec)
    res['num_h'] = _numerators(em, em.step_h, 'h', Vn, prec)
    # the step, emulated from the device's own slabs
    em.em_step(tW, tH, tZ, aW, aH, aZ)
    torch.cuda.synchronize()
    sw, sh = _slab_planes(em.step_w, R), _slab_planes(em.step_h, R)
    kW, kH = P.chain_rows(C, r_pad), P.chain_rows(N, r_pad)
    ref = P.em_step(W0, H0, Z0, sw, sh, train, alphas, kW=kW, kH=kH)
    W1, H1, Z1 = _np(em.W), _np(em.H), _np(em.Z)
    for key, new, old, t in (('W', W1, W0, tW), ('H', H1, H0, tH), ('Z', Z1, Z0, tZ)):
        if t:
            res[key] = P.excess(new, ref[key])
        else:
            assert np.array_equal(new.view(np.uint32), old.view(np.uint32)), key
    # column sums: what the emulated columns sum to, and 1 where the update normalises by a sum of the same terms
    nslab = max(em.step_w.nsplit, em.step_h.nsplit)
    for key, new, t, k, alpha, own in (('W', W1, tW, kW, aW, True), ('H', H1, tH, kH, aH, not tW and not tZ)):
        if t:
            s = new.astype(np.float64).sum(0)
            res[key + '_colsum'] = P.excess(s, P.Val(ref[key].v.sum(0), ref[key].e.sum(0)))
            if alpha != 1 or own:
                res[key + '_unit'] = float(np.abs(s - 1).max() / P.unit_sum_bound(k, nslab))
    if tZ:
        res['Z_unit'] = float(abs(Z1.astype(np.float64).sum() - 1) / (P.SECOND * (P.CHAIN_Z + 1) * P.U))
    # the float64 oracle from the old masters
    t64 = lambda a: torch.from_numpy(np.asarray(a, dtype=np.float64))
    Wr, Hr, Zr = O.plca_em_step(t64(Vn), t64(W0), t64(H0), t64(Z0), aW, aH, aZ, train=train)
    res['oracle'] = max(rel_err(W1, Wr), rel_err(H1, Hr), rel_err(Z1, Zr))
    return res


@pytest.mark.parametrize('i', range(len(P.DENSE_CASES)), ids=lambda i: P.dense_id(P.DENSE_CASES[i]))
def test_dense_em_steps_per_element(dev, monkeypatch, i):
    from torchnmf_amd.plca import _PlcaEM
    case = P.DENSE_CASES[i]
    monkeypatch.delenv('TORCHNMF_AMD_NSPLIT', raising=False)
    if case['nsplit']:
        monkeypatch.setenv('TORCHNMF_AMD_NSPLIT', str(case['nsplit']))
    Vn, W0, H0, Z0 = P.dense_problem(case)
    em = _PlcaEM(_up(Vn, dev), _up(W0, dev), _up(H0, dev), _up(Z0, dev), case['precision'])
    prec = em.precision_name
    assert prec == (case['precision'] or ('bf16x3' if P.pad_rank(case['R']) <= 128 else 'bf16'))
    if case['nsplit']:
        assert em.step_w.nsplit == case['nsplit'] and em.step_h.nsplit == case['nsplit']
    tol, bar = E.TOL[prec], (1e-4 if prec == 'bf16x3' else 2e-2)
    out = []
    start = [(em.W, _up(W0, dev)), (em.H, _up(H0, dev)), (em.Z, _up(Z0, dev))]
    for train, alphas in P.dense_steps(i):
        # every step from the case's start state (plca_emulation.split_plane_sensitivity: after an alpha = 0.99 step the
        # EMULATION of the bf16x3 numerators is ambiguous beyond TOL -- 5.3e-6 was measured there against 4e-6)
        for p_, v in start:
            p_.copy_(v)
        em.repack()
        r = _dense_em_step(em, Vn, prec, train, alphas)
        tag = ''.join(n for n, t in zip('WHZ', train) if t)
        record('plca_emulated_parity', kernel='dense_em_step', case=P.dense_id(case), train=tag, alphas=alphas, tol=tol,
               nsplit=(em.step_w.nsplit, em.step_h.nsplit), **r)
        print(P.dense_id(case), tag, alphas, r)
        out.append((tag, alphas, r))
    for tag, alphas, r in out:
        assert r['image_mismatch'] == 0, (tag, alphas, r)
        for w in ('num_w', 'num_h'):
            assert r[w]['err'] <= tol and r[w]['nan_left'] == 0 and r[w]['negative'] == 0, (tag, alphas, w, r[w])
        for key in ('W', 'H', 'Z', 'W_colsum', 'H_colsum', 'W_unit', 'H_unit', 'Z_unit', 'loss'):
            assert r.get(key, 0.0) <= 1.0, (tag, alphas, key, r)
        assert r['oracle'] < bar, (tag, alphas, r['oracle'])


@pytest.mark.parametrize('M,K,R,nsplit', [(200, 330, 40, 1), (300, 520, 200, 2)], ids=['r_pad64', 'r_pad256-split'])
def test_split_panel_kernel_with_f16_operands_at_the_abi(dev, lib, M, K, R, nsplit):
    """fused_kernel<kKL, kPrecF16, kModeMU2>: no model reaches it (PLCA refuses fp16 operands), nmfmu_mu_partial exports it."""
    from torchnmf_amd import _capi
    from torchnmf_amd.engine import DEFAULT_BACKEND_FACTORY, FactorBuf, StepBuf, _ptr
    be = DEFAULT_BACKEND_FACTORY()
    prec, pc = 'f16', _capi.PREC_F16
    r_pad = be.pad_rank(R)
    g = torch.Generator().manual_seed(M + K + R)
    X = torch.rand(M, K, generator=g)
    X = torch.where(torch.rand(M, K, generator=g) < 0.1, torch.zeros(()), X)
    A = torch.randn(M, R, generator=g).abs() + 0.05
    B = torch.randn(K, R, generator=g).abs() + 0.05
    z = torch.rand(R, generator=g) + 0.25
    fA, fB, fBz = (FactorBuf(t.clone().to(dev), r_pad, pc, be) for t in (A, B, B))
    zs, ones = _padded_vec(z.numpy(), r_pad, dev), torch.ones(r_pad, dtype=torch.float32, device=dev)
    for fb, sc in ((fA, ones), (fB, ones), (fBz, zs)):
        assert lib.nmfmu_pack_factor_scaled(ctypes.byref(fb.struct), R, r_pad, pc, sc.data_ptr(), _s()) == 0
    torch.cuda.synchronize()
    assert not any(G._check_images(fA, r_pad, prec, False).values()) and not any(G._check_images(fB, r_pad, prec, False).values())
    assert not any(G._check_images(_shim(fBz, (B * z[None, :]).numpy()), r_pad, prec, False).values())
    m_pad, k_pad = fA.rows_pad, fB.rows_pad
    xp = be.pack_x(X.to(dev), False, pc, 128, m_pad, k_pad, None)
    assert nsplit <= k_pad // 64 // 4 or nsplit == 1
    st = StepBuf(xp, fA, fB, R, r_pad, nsplit, pc, _capi.STAGE_DMA_SPLIT, 128, 1.0, 1.0, 0.0, 0.0, need_den=False)
    st.struct.panel.p1_hi = _ptr(fBz.p1_hi)
    st.slab_num.fill_(NAN)
    be.mu_partial(st)
    torch.cuda.synchronize()
    num = st.slab_num.view(nsplit, m_pad, r_pad).double().sum(0).cpu().numpy()[:M, :R]
    hs = E.half_step(X.numpy(), None, None, 1.0, prec, A_img=_img(fA, r_pad, prec, M, R), B_img=_img(fBz, r_pad, prec, K, R),
                     B2_img=_img(fB, r_pad, prec, K, R))
    err, raw = float(E.elem_err(num, hs['num'], hs['num_amb']).max()), float(E.elem_err(num, hs['num']).max())
    record('plca_emulated_parity', kernel='kModeMU2-f16', shape=(M, K, R), nsplit=nsplit, err=err, raw=raw, tol=E.TOL[prec])
    print(M, K, R, err, raw)
    assert err <= E.TOL[prec]


# ---- c. one EM step on the convolutive engine --------------------------------------------------------------------------
def _conv_em_step(em, Vn, W0, H0, Z0, train, alphas):
    import conv_emulation as CE
    import test_gpu_conv_emulated_parity as GC
    from oracle import mu_oracle as O
    e = em.eng
    prec = e.precision_name
    C, B, R, T = e.C, e.B, e.R, e.T
    BL, RT = B * e.L, R * T
    rview = (1, R) + (1,) * (W0.ndim - 2)
    res = {}
    scaled = lambda W, Z: (W * Z.reshape(rview)).astype(np.float32)                    # one fp32 multiply, as the pack kernel's
    wm_bad = lambda W, Z: (GC._image_mismatch(em.wm_s, GC._padded(scaled(W, Z).reshape(C, -1), e.c_pad, e.rp_pad), prec)
                           + GC._image_mismatch(em.wmt_s, GC._padded(scaled(W, Z).reshape(C, -1).T, e.rp_pad, e.c_pad), prec))
    res['wm_s_before'] = wm_bad(W0, Z0)
    rz = bool(e.c_rows)
    GC._poison(e, ('gn',), C, BL, prec, rz)
    GC._poison(e, ('gnt',), BL, C, prec, rz)
    e.num_w.fill_(NAN)
    em.numh.fill_(NAN)
    em.em_step(*train, *alphas)
    torch.cuda.synchronize()
    # the ratio words the device wrote, held to the emulated rounding one by one, then contracted as they are
    ops_s, ops = CE.operands(scaled(W0, Z0), H0, prec), CE.operands(W0, H0, prec)
    rt = CE.ratio(CE.target_w(Vn), ops_s, 1.0, prec)
    pw, ph = GC._read_planes(e, {'gn': 'gn'}), GC._read_planes(e, {'gn': 'gnt'})
    res['ratio_w'] = CE.check_ratio(pw, rt, prec, 1.0, e.c_rows)
    res['ratio_h'] = CE.check_ratio(ph, rt, prec, 1.0, e.c_rows, transpose=True)
    nw = CE.numerators_w(CE.with_device_planes(rt, pw, prec), ops)
    nh = CE.numerators_h(CE.with_device_planes(rt, ph, prec, True), ops, B)
    rows = e.c_rows or e.c_pad
    numw = e.num_w[:rows * e.rp_pad].view(rows, e.rp_pad)[:C, :RT].double().cpu().numpy()
    numh = em.numh.view(H0.shape).double().cpu().numpy()
    res['num_w'], res['num_w_raw'] = CE.value_err(numw, nw['num'], nw['num_amb'])
    res['num_h'], res['num_h_raw'] = CE.value_err(numh, nh['num'], nh['num_amb'])
    # the update from the device's own numerators
    ref = P.em_step(W0, H0, Z0, numw.reshape(W0.shape), numh, train, alphas, kW=P.chain_plca3(C, T), kH=P.chain_plca3(B, e.Lh),
                    kZ=max(R - 1, 1))
    W1, H1, Z1 = _np(em.W), _np(em.H), _np(em.Z)
    for key, new, old, t in (('W', W1, W0, train[0]), ('H', H1, H0, train[1]), ('Z', Z1, Z0, train[2])):
        if t:
            res[key] = P.excess(new, ref[key])
        else:
            assert np.array_equal(new.view(np.uint32), old.view(np.uint32)), key
    # an exact zero of W stays one -- unless W takes a Dirichlet prior, which lifts it to max(alpha - 1, eps) / colsum (the W check)
    assert (W0 == 0).any()
    res['zeros_kept'] = bool((W1[W0 == 0] == 0).all()) if (not train[0] or alphas[0] == 1) else None
    res['wm_s_after'] = wm_bad(W1, Z1)
    t64 = lambda a: torch.from_numpy(np.asarray(a, dtype=np.float64))
    Wr, Hr, Zr = O.plca_em_step(t64(Vn), t64(W0), t64(H0), t64(Z0), *alphas, train=train)
    res['oracle'] = max(rel_err(W1, Wr), rel_err(H1, Hr), rel_err(Z1, Zr))
    return res


@pytest.mark.parametrize('i', range(len(P.CONV_CASES)), ids=lambda i: P.conv_id(P.CONV_CASES[i]))
def test_conv_em_steps_per_element(dev, monkeypatch, i):
    import conv_emulation as CE
    from torchnmf_amd.plca import _ConvPlcaEM
    case = P.CONV_CASES[i]
    for k in ('WINSTAGE', 'EXPLICIT', 'H_ROWS', 'H_FOLD', 'KSPLIT', 'NARROW'):
        monkeypatch.delenv('TORCHNMF_AMD_NMFD_' + k, raising=False)
    monkeypatch.setenv('TORCHNMF_AMD_NMFD_H_ROWS', case['h_rows'])
    Vn, W0, H0, Z0 = P.conv_problem(case)
    em = _ConvPlcaEM(_up(Vn, dev), _up(W0, dev), _up(H0, dev), _up(Z0, dev), None)
    e = em.eng
    prec = e.precision_name
    assert prec == 'bf16x3' and bool(e.h_rows) == (case['h_rows'] == '1')
    if case['shape'] == P.CONV_KSPLIT_SHAPE:
        assert e.w_ksplit > 1                                         # num_w is read after nmfmu_slab_sum
    tol = E.TOL[prec]
    start = [(em.W, _up(W0, dev)), (em.H, _up(H0, dev)), (em.Z, _up(Z0, dev))]
    out = []
    for train, alphas in P.conv_steps(i):
        for p_, v in start:
            p_.copy_(v)
        em.repack()
        r = _conv_em_step(em, Vn, W0, H0, Z0, train, alphas)
        tag = ''.join(n for n, t in zip('WHZ', train) if t)
        record('plca_emulated_parity', kernel='conv_em_step', case=P.conv_id(case), train=tag, alphas=alphas, tol=tol,
               w_ksplit=e.w_ksplit, h_rows=bool(e.h_rows), implicit=bool(e.implicit), c_rows=e.c_rows, **r)
        print(P.conv_id(case), tag, alphas, r)
        out.append((tag, alphas, r))
    for tag, alphas, r in out:
        assert r['wm_s_before'] == 0 and r['wm_s_after'] == 0 and r['zeros_kept'] in (True, None), (tag, alphas, r)
        assert CE.ratio_ok(r['ratio_w']) and CE.ratio_ok(r['ratio_h']), (tag, alphas, r)
        assert r['num_w'] <= tol and r['num_h'] <= tol, (tag, alphas, r)
        for key in ('W', 'H', 'Z'):
            assert r.get(key, 0.0) <= 1.0, (tag, alphas, key, r)
        assert r['oracle'] < 1e-4, (tag, alphas, r['oracle'])
