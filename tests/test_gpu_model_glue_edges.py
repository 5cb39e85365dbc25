"""
GPU tests of the model-level glue at the bottom of csrc/elbo.hip — model_prepare_kernel (dpgp_model_prepare, dpgp_model_prepare_t),
model_backward_kernel (dpgp_model_backward, dpgp_model_backward_t), model_pack_kernel / model_finalize_kernel and their two fused copies
(sum_terms_body in linalg.hip, the end of fhat_t_combine_kernel), trouble_flag_kernel — called directly through the C ABI, at every
grid role, cap, chunk, pass and wave edge of their launch arithmetic and over the whole range of their hand-written special functions.

The reference is tests/test_model_glue_refs.restate (torch fp64 + autograd, special functions from mpmath; pinned there against 60-digit
mpmath to 1e-14 max(1, max |value|)).  f_hat is a linear surrogate: its fixed signed coefficients are the df_d* inputs of backward.

Tolerance: 1e-12 max(1, max |reference| over the compared block) — the project's figure for an fp64 operator against its CPU restatement
(test_gpu_predict_b1.close) — per output array, for [D, .] and [N, Q] arrays per block of 64 rows; scalars relative to the sum of
|terms| the restatement returns.  Every case is launched twice and must give equal bits.  Each test prints its family's largest error per
output as a fraction of the tolerance (DESIGN.md 7.23 holds the table).
"""
import functools

import numpy as np
import pytest
import torch

import test_model_glue_refs as R
from dp_gp_lvm_amd import _lib, ops

pytestmark = pytest.mark.gpu

F64 = torch.float64
TOL = 1e-12
BLOCK_ROWS = 64
FORMS = ('d', 't')


# ---------------------------------------------------------------------------------------------------------------
# launching
# ---------------------------------------------------------------------------------------------------------------
def _up(a, dev):
    return torch.tensor(np.asarray(a), dtype=F64, device=dev)


def _nan(shape, dev):
    return torch.full(shape if isinstance(shape, tuple) else (shape,), float('nan'), dtype=F64, device=dev)


def run_glue(dev, c, form, D=None, d_offset=None, add_constants=None, adj=None, phi_out=True):
    """dpgp_model_prepare[_t] then dpgp_model_backward[_t] (fed the phi prepare stored, as the models do) -> dict of NumPy arrays named
    as R.restate names them.  Outputs start as NaN, d_logits as garbage (the entry point clears it)."""
    l, st = _lib.lib(), torch.cuda.current_stream().cuda_stream
    D = c.D if D is None else D
    d_offset = c.d_offset if d_offset is None else d_offset
    cc = int(c.add_constants if add_constants is None else add_constants)
    T, Q, N, M = c.T, c.Q, c.N, c.M
    raw = {k: _up(c.raw[k], dev) for k in R.RAW_NAMES}
    A = {k: _up(v, dev) for k, v in (c.adj[form] if adj is None else adj).items()}
    p = lambda t_: t_.data_ptr()
    ins = [p(raw[k]) for k in ('logits', 'gat_raw', 'aat_raw', 'bat_raw', 's_raw', 'g1_raw', 'g2_raw', 'w_raw')]
    s, phi, scal = _nan((N, Q), dev), _nan((D, T), dev), _nan(l.dpgp_model_scal_count(D), dev)
    out = {}
    if form == 'd':
        gamma, alpha, beta = _nan((D, Q), dev), _nan(D, dev), _nan(D, dev)
        _lib.check(l.dpgp_model_prepare(D, T, Q, N, d_offset, c.mask_size, *ins, c.s1, c.s2, cc, p(gamma), p(alpha), p(beta), p(s),
                                        p(phi) if phi_out else None, p(scal), st), 'dpgp_model_prepare')
        out.update(gamma=gamma, alpha=alpha, beta=beta)
    else:
        atoms = _nan(T * Q + 2 * T, dev)
        _lib.check(l.dpgp_model_prepare_t(D, T, Q, N, d_offset, c.mask_size, *ins, c.s1, c.s2, cc, p(s), p(phi), p(atoms), p(scal),
                                          st), 'dpgp_model_prepare_t')
        out.update(atoms=atoms)
    out.update(s=s, scal=scal)
    if phi_out:
        out['phi'] = phi
        nm1 = max(T - 1, 1)
        g = dict(d_x_mean=_nan((N, Q), dev), d_s_raw=_nan((N, Q), dev), d_x_u=_nan((M, Q), dev),
                 d_logits=torch.full((c.rows, T), 3.25, dtype=F64, device=dev), d_g1_raw=_nan(nm1, dev), d_g2_raw=_nan(nm1, dev),
                 d_w_raw=_nan(2, dev), d_gat_raw=_nan((T, Q), dev), d_aat_raw=_nan(T, dev), d_bat_raw=_nan(T, dev))
        head = [D, T, Q, N, M, d_offset, c.mask_size, c.rows] + ins + [p(raw['x_mean']), p(phi), c.s1, c.s2, cc]
        df = [p(A[k]) for k in ('A_mu', 'A_s', 'A_z', 'A_g', 'A_ab')]
        outs = [p(g[k]) for k in R.GRAD_NAMES]
        if form == 'd':
            _lib.check(l.dpgp_model_backward(*head, *df, *outs, st), 'dpgp_model_backward')
        else:
            _lib.check(l.dpgp_model_backward_t(*head, *df, p(A['A_phi']), *outs, st), 'dpgp_model_backward_t')
        out.update(g)
    torch.cuda.synchronize()
    res = {k: v.cpu().numpy() for k, v in out.items()}
    if T == 1:
        res['d_g1_raw'], res['d_g2_raw'] = np.zeros(0), np.zeros(0)
    return res


@functools.lru_cache(maxsize=None)
def reference(c, form, D=None, d_offset=None, add_constants=None):
    ref = R.restate(c, form, D=D, d_offset=d_offset, add_constants=add_constants)
    for v in ref.values():
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
    return ref


# ---------------------------------------------------------------------------------------------------------------
# comparing
# ---------------------------------------------------------------------------------------------------------------
ARRAYS = ('gamma', 'alpha', 'beta', 'atoms', 's', 'phi') + R.GRAD_NAMES
FAMILY = {}


def _array_fraction(got, ref):
    got, ref = np.asarray(got, dtype=np.float64), np.asarray(ref, dtype=np.float64)
    assert got.shape == ref.shape, (got.shape, ref.shape)
    if ref.size == 0:
        return 0.0
    blocks = [slice(None)] if ref.ndim < 2 else [slice(i, i + BLOCK_ROWS) for i in range(0, ref.shape[0], BLOCK_ROWS)]
    worst = 0.0
    for b in blocks:
        fr = np.max(np.abs(got[b] - ref[b])) / (TOL * max(1.0, float(np.max(np.abs(ref[b])))))
        worst = fr if not fr <= worst else worst          # (NaN is kept)
    return float(worst)


def fractions(got, ref):
    """{output: largest error / tolerance} over everything `got` holds."""
    fr = {k: _array_fraction(got[k], ref[k]) for k in ARRAYS if k in got}
    sc = got['scal']
    fr['scal0'] = abs(sc[0] - ref['scal0']) / (TOL * max(1.0, ref['scal0_abs']))
    fr['hyper'] = abs(sc[1] - ref['hyper']) / (TOL * max(1.0, ref['hyper_abs']))
    assert sc.shape[0] == 2 + ref['rows'].shape[0]
    fr['rows'] = float(np.max(np.abs(sc[2:] - ref['rows']) / (TOL * np.maximum(1.0, ref['rows_abs']))))
    return fr


def note(family, fr):
    fam = FAMILY.setdefault(family, {})
    for k, v in fr.items():
        old = fam.get(k, 0.0)
        fam[k] = old if v <= old else v                   # (NaN is kept)


def same_bits(a, b):
    assert a.keys() == b.keys()
    for k in a:
        assert a[k].tobytes() == b[k].tobytes(), 'two launches differ in ' + k


def check(dev, family, c, forms=FORMS, finite_only=(), **kw):
    """Both forms of one case: launched twice (equal bits), every output within the tolerance of the restatement.  finite_only: (form,
    output) pairs that are only required to be finite (the restatement cannot judge them)."""
    res = {}
    for form in forms:
        got = run_glue(dev, c, form, **kw)
        same_bits(got, run_glue(dev, c, form, **kw))
        fr = fractions(got, reference(c, form, **kw))
        for f_, k in finite_only:
            if f_ == form:
                assert np.all(np.isfinite(got[k])), (c.name, form, k)
                del fr[k]
        note(family, fr)
        bad = {k: v for k, v in fr.items() if not v <= 1.0}
        assert not bad, (c.name, form, bad)
        res[form] = got
    return res


def report(family):
    print('\n%s largest error / tolerance: %s' % (family, '  '.join('%s %.3g' % kv for kv in sorted(FAMILY.get(family, {}).items()))))


# ---------------------------------------------------------------------------------------------------------------
# G1 — row blocks of prepare
# ---------------------------------------------------------------------------------------------------------------
G1 = [(D, 5, 4) for D in (1, 15, 16, 17, 33)] + [(17, 5, Q) for Q in (1, 14, 15, 16, 30)] + \
     [(17, T, 4) for T in (1, 2, 21, 22, 64)] + [(33, 64, 30)]


@pytest.mark.parametrize('D,T,Q', G1, ids=['D%d-T%d-Q%d' % x for x in G1])
def test_g1_prepare_row_blocks(dev, D, T, Q):
    c = R.make_case('g1', D=D, T=T, Q=Q, seed=11)
    m = c.mirror()
    assert m['nrb'] == (D + 15) // 16 and m['row_elems_per_thread'] == (2 if Q >= 16 else 1)
    assert m['digamma_last_thread'] == {1: None, 2: 66, 5: 75, 21: 123, 22: 126, 64: 252}[T]
    got = check(dev, 'G1', c)
    null = run_glue(dev, c, 'd', phi_out=False)                  # phi_out = nullptr: the same gamma, alpha, beta, s and scalars
    for k in null:
        assert null[k].tobytes() == got['d'][k].tobytes(), k
    report('G1')


# ---------------------------------------------------------------------------------------------------------------
# G2 — block 0 of backward
# ---------------------------------------------------------------------------------------------------------------
G2 = [(5, 15, 14, 255, 1, 1), (5, 8, 29, 256, 1, 1), (5, 64, 1, 256, 1, 1), (5, 9, 29, 288, 2, 1), (70, 9, 29, 288, 2, 2),
      (5, 64, 30, 2112, 9, 1), (127, 5, 4, 35, 1, 1), (128, 5, 4, 35, 1, 1), (129, 5, 4, 35, 1, 2), (257, 5, 4, 35, 1, 3),
      (32, 64, 4, 448, 2, 1), (33, 64, 4, 448, 2, 2), (65, 64, 4, 448, 2, 3), (5, 2, 4, 14, 1, 1), (130, 5, 30, 165, 1, 3)]


@pytest.mark.parametrize('D,T,Q,elems,passes,chunks', G2, ids=['D%d-T%d-Q%d' % x[:3] for x in G2])
def test_g2_backward_block0(dev, D, T, Q, elems, passes, chunks):
    """T (Q + 3) = 255 | 256 | 288 and up to nine e0 passes; D on both sides of DC and 2 DC at DC = 128 (T = 5, Q = 4), DC = 32 (T = 64),
    DC = 64 (two passes AND two chunks) and DC = 62 (Q = 30: no power of two); stail at T = 2."""
    c = R.make_case('g2', D=D, T=T, Q=Q, seed=12)
    m = c.mirror()
    assert (m['block0_elems'], m['e0_passes'], m['dc_chunks']) == (elems, passes, chunks)
    assert m['DC'] == {(5, 4): 128, (64, 4): 32, (9, 29): 64, (5, 30): 62}.get((T, Q), m['DC'])
    check(dev, 'G2', c)
    report('G2')


# ---------------------------------------------------------------------------------------------------------------
# G3 — logits rows
# ---------------------------------------------------------------------------------------------------------------
G3 = [(5, 1, 0, 0), (6, 2, 0, 0), (7, 2, 0, 0), (9, 3, 0, 0), (10, 3, 0, 0), (14, 7, 0, 0), (15, 7, 0, 0), (7, 3, 3, 0), (7, 3, 4, 0),
      (7, 3, 4, 2), (5, 1, 0, 3), (256, 1, 0, 0), (257, 1, 0, 0), (513, 2, 0, 1), (513, 2, 3, 1)]


@pytest.mark.parametrize('D,mask,off,extra', G3, ids=['D%d-m%d-o%d-x%d' % x for x in G3])
def test_g3_logits_rows(dev, D, mask, off, extra):
    c = R.make_case('g3', D=D, T=3, Q=2, mask_size=mask, d_offset=off, extra_rows=extra, seed=13)
    m = c.mirror()
    r0, r1 = off // mask, (off + D - 1) // mask
    assert m['rows'] == r1 - r0 + 1 and m['nlb'] == (2 if m['rows'] > 256 else 1) and c.rows == r1 + 1 + extra
    if (D, mask, off) == (7, 3, 4):
        assert (r0, r1) == (1, 3) and off % mask and (off + D) % mask      # first and last groups partial
    got = check(dev, 'G3', c)
    for form in FORMS:
        dl = got[form]['d_logits']
        assert np.all(dl[:r0] == 0.0) and np.all(dl[r1 + 1:] == 0.0) and not np.any(np.signbit(dl[:r0]))
        assert np.all(dl[r0:r1 + 1] != 0.0)
    report('G3')


@pytest.mark.parametrize('bounds', [(0, 7, 20), (0, 5, 13, 20), (0, 1, 20)], ids=['world2', 'world3', 'world2-one'])
def test_g3_shard_sums(dev, bounds):
    """The ranks' partial forward scalars and ten partial gradient arrays (add_constants on rank 0 only, every rank with adjoints of
    its own) add up to the one-rank call on the summed adjoints; every rank also meets the restatement.  mask_size = 3: the splits
    cut mask groups, whose logits row then collects from two ranks."""
    D, mask = 20, 3
    assert any(b % mask for b in bounds[1:-1])
    base = R.make_case('g3s', D=D, T=4, Q=3, N=5, M=3, mask_size=mask, seed=14)
    world = len(bounds) - 1
    rng = np.random.default_rng(15)
    for form in FORMS:
        full_adj = base.adj[form]
        shared = ('A_mu', 'A_s', 'A_z') + (('A_g', 'A_ab') if form == 't' else ())
        parts = []
        for r in range(world):
            lo, hi = bounds[r], bounds[r + 1]
            adj = {k: (rng.standard_normal(v.shape) if k in shared else v[lo:hi].copy()) for k, v in full_adj.items()}
            parts.append((lo, hi, adj))
        total = {k: (sum(a[k] for _, _, a in parts) if k in shared else v) for k, v in full_adj.items()}
        one_case = R.Case('g3s-one', D, base.T, base.Q, base.N, base.M, mask, 0, base.rows, 1, base.s1, base.s2,
                          {k: v.copy() for k, v in base.raw.items()}, {form: {k: v.copy() for k, v in total.items()}})
        one = check(dev, 'G3', one_case, forms=(form,))[form]
        ref = reference(one_case, form)
        acc = {k: np.zeros_like(one[k]) for k in R.GRAD_NAMES}
        dp_sum = 0.0
        for r, (lo, hi, adj) in enumerate(parts):
            rank_case = R.Case('g3s-rank', hi - lo, base.T, base.Q, base.N, base.M, mask, lo, base.rows, int(r == 0), base.s1, base.s2,
                               {k: v.copy() for k, v in base.raw.items()}, {form: adj})
            got = check(dev, 'G3', rank_case, forms=(form,))[form]
            for k in acc:
                acc[k] += got[k]
            dp_sum += got['scal'][0] + np.sum(got['scal'][2:])
            assert (got['scal'][0] == 0.0) == (r != 0) and got['scal'][1] == one['scal'][1]
        for k in acc:
            fr = _array_fraction(acc[k], one[k])
            assert fr <= 1.0, (form, k, fr)
        dp_abs = ref['scal0_abs'] + float(np.sum(ref['rows_abs']))
        assert abs(dp_sum - (one['scal'][0] + np.sum(one['scal'][2:]))) <= TOL * max(1.0, dp_abs)
    report('G3')


# ---------------------------------------------------------------------------------------------------------------
# G4 — element-wise parts
# ---------------------------------------------------------------------------------------------------------------
G4 = [(1, 1, 1), (255, 1, 2), (17, 15, 2), (256, 1, 2), (16, 16, 2), (257, 1, 2), (8739, 30, 2), (34950, 30, 3)]


@pytest.mark.parametrize('N,Q,M', G4, ids=['N%d-Q%d-M%d' % x for x in G4])
@pytest.mark.parametrize('cc', [1, 0])
def test_g4_elementwise(dev, N, Q, M, cc):
    """N Q = 1 | 255 | 256 | 257, one case past the 512-block cap of prepare's softplus part (N Q > 512 * 512: a third trip of its stride
    loop) and one past the 1024-block cap of backward's element-wise part ((N + M) Q > 1024 * 1024: a fifth trip)."""
    c = R.make_case('g4', D=3, T=2, Q=Q, N=N, M=M, add_constants=cc, seed=16)
    m = c.mirror()
    if N == 8739:
        assert m['sblocks_capped'] and m['sblocks'] == 512 and m['s_trips'] == 3 and N * Q * 8 < 10e6
    elif N == 34950:
        assert m['neb_capped'] and m['neb'] == 1024 and m['e_trips'] == 5 and (N + M) * Q * 8 < 10e6
    else:
        assert N * Q in (1, 255, 256, 257) and not m['sblocks_capped'] and not m['neb_capped']
    got = check(dev, 'G4', c)
    for form in FORMS:
        g, A = got[form], c.adj[form]
        assert np.array_equal(g['d_x_u'], -A['A_z'])
        if cc == 0:                                                   # no KL, no hyper-prior, no DP constants: exactly
            assert np.array_equal(g['d_x_mean'], -A['A_mu']) and g['scal'][0] == 0.0 and np.all(g['d_w_raw'] == 0.0)
            sig = 1.0 / (1.0 + np.exp(-c.raw['s_raw']))
            assert np.max(np.abs(g['d_s_raw'] + A['A_s'] * sig)) <= 4 * np.finfo(np.float64).eps * np.max(np.abs(A['A_s']))
    report('G4')


# ---------------------------------------------------------------------------------------------------------------
# G5 — range
# ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('name', R.g5_names())
def test_g5_range(dev, name):
    """Each raw family at -30 ... 30 and 700 (softplus arguments from 1e-13 to 700 through digamma, trigamma and lgamma, on both sides
    of each recurrence stop), logit rows of spread 0 ... 600, and 800, where phi underflows to 0 and the row's gradient is its finite
    limit.  tests/test_model_glue_refs.py holds the restatement to 1e-14 against mpmath on these very inputs."""
    c = R.g5_case(name)
    # a left-out (case, form) still runs: equal bits, every other output against the restatement, d_logits finite
    got = check(dev, 'G5', c, finite_only=tuple((f, R.G5_LEFT_OUT[(n, f)]) for n, f in R.G5_LEFT_OUT if n == name))
    if name == 'spread=800':
        assert all(np.any(got[f]['phi'] == 0.0) and np.all(np.isfinite(got[f]['d_logits'])) for f in FORMS)
    report('G5')


# ---------------------------------------------------------------------------------------------------------------
# G6 — the tails
# ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('D', [15, 16, 17, 33])
def test_g6_tails(dev, D):
    """dpgp_model_pack + dpgp_model_finalize against the fused tails of dpgp_elbo_fhat (sum_terms_body) and dpgp_elbo_fhat_t
    (fhat_t_combine_kernel): equal bits, and out = (objective, f_hat, KL, DP objective, hyper-prior) with the restatement's DP objective
    and hyper-prior and objective = dp - (f_hat - KL) - hyper."""
    l, st = _lib.lib(), torch.cuda.current_stream().cuda_stream
    N, M, Q, T = 20, 8, 2, 4
    c = R.make_case('g6', D=D, T=T, Q=Q, N=N, M=M, seed=17)
    rng = np.random.default_rng(18)
    y = _up(rng.standard_normal((N, D)), dev)
    z, mu = _up(c.raw['x_u'], dev), _up(c.raw['x_mean'], dev)
    for form in FORMS:
        got = run_glue(dev, c, form)
        ref = reference(c, form)
        scal, s = _up(got['scal'], dev), _up(got['s'], dev)
        pack_f, out_f = _nan(2, dev), _nan(5, dev)
        if form == 'd':
            _, sums, _ = ops.elbo_fhat(y, z, mu, s, _up(got['gamma'], dev), _up(got['alpha'], dev), _up(got['beta'], dev), prec='f64',
                                       model_tail=(scal, pack_f, out_f))
        else:
            at = _up(got['atoms'], dev)
            _, _, sums, _ = ops.elbo_fhat_t(y, torch.sum(y * y, dim=0), z, mu, s, at[:T * Q].view(T, Q), at[T * Q:T * Q + T],
                                            at[T * Q + T:], _up(got['phi'], dev).t(), prec='f64', model_tail=(scal, pack_f, out_f))
        pack, out = _nan(2, dev), _nan(5, dev)
        _lib.check(l.dpgp_model_pack(D, sums.data_ptr(), scal.data_ptr(), pack.data_ptr(), st), 'dpgp_model_pack')
        _lib.check(l.dpgp_model_finalize(pack.data_ptr(), sums[1:2].data_ptr(), scal[1:2].data_ptr(), out.data_ptr(), st),
                   'dpgp_model_finalize')
        torch.cuda.synchronize()
        pack, out, pack_f, out_f, sums = (a.cpu().numpy() for a in (pack, out, pack_f, out_f, sums))
        assert pack.tobytes() == pack_f.tobytes() and out.tobytes() == out_f.tobytes(), (form, pack, pack_f, out, out_f)
        fhat, kl = sums
        assert np.isfinite(fhat) and np.isfinite(kl) and pack[0] == fhat and out[1] == fhat and out[2] == kl
        dp_abs = max(1.0, ref['scal0_abs'] + float(np.sum(ref['rows_abs'])))
        fr = dict(dp=abs(out[3] - ref['dp']) / (TOL * dp_abs), pack=abs(pack[1] - ref['dp']) / (TOL * dp_abs),
                  hyper=abs(out[4] - ref['hyper']) / (TOL * max(1.0, ref['hyper_abs'])),
                  objective=abs(out[0] - (ref['dp'] - (fhat - kl) - ref['hyper']))
                  / (TOL * (dp_abs + abs(fhat) + abs(kl) + max(1.0, ref['hyper_abs']))))
        note('G6', fr)
        assert all(v <= 1.0 for v in fr.values()), (form, fr)
    report('G6')


# ---------------------------------------------------------------------------------------------------------------
# G7 — the trouble flag
# ---------------------------------------------------------------------------------------------------------------
G7_N = (1, 1023, 1024, 1025, 8192, 8193, 256 * 8192, 256 * 8192 + 1025)


@pytest.mark.parametrize('n', G7_N)
def test_g7_trouble_flag(dev, n):
    l, st = _lib.lib(), torch.cuda.current_stream().cuda_stream
    m = R.flag_mirror(n, 4)
    assert m['grid'] == min(256, (n + 8191) // 8192) and m['capped'] == (n > 256 * 8192)
    assert m['trips'] == dict(zip(G7_N, (1, 1, 1, 2, 8, 5, 8, 9)))[n]
    rng = np.random.default_rng(19)
    flat = _up(rng.standard_normal(n + 1), dev)
    flat[n] = float('nan')                                            # the word just behind the scanned range
    info = torch.zeros(4, dtype=torch.int32, device=dev)
    out = _nan(1, dev)

    def flag(n_=n, d=4, info_=info):
        _lib.check(l.dpgp_trouble_flag(n_, flat.data_ptr(), d, None if info_ is None else info_.data_ptr(), out.data_ptr(), st),
                   'dpgp_trouble_flag')
        v = float(out.item())
        assert v in (0.0, 1.0)
        out.fill_(float('nan'))
        return v

    assert flag() == 0.0
    spots = sorted({0, n - 1} | ({m['stride']} if m['stride'] < n else set()))
    if n == G7_N[-1]:
        assert m['stride'] == 256 * 1024 and 8 * m['stride'] in range(n)          # (the ninth trip exists only for the first 1025 words)
        spots.append(8 * m['stride'])
    for i in spots:
        for bad in (float('nan'), float('inf'), float('-inf')):
            keep = float(flat[i])
            flat[i] = bad
            assert flag() == 1.0, (i, bad)
            flat[i] = keep
            assert flag() == 0.0
    for i in (0, 3):
        info[i] = -7 if i else 5
        assert flag() == 1.0
        info[i] = 0
    assert flag(d=0, info_=None) == 0.0
    big = torch.zeros(n + 9000, dtype=torch.int32, device=dev)       # d > n: the info words set the grid
    assert R.flag_mirror(n, n + 9000)['grid'] >= m['grid'] and flag(d=n + 9000, info_=big) == 0.0
    big[n + 8999] = 1
    assert flag(d=n + 9000, info_=big) == 1.0
    assert flag(d=n + 8999, info_=big) == 0.0


def test_scal_count_matches_the_mirror(dev):
    l = _lib.lib()
    for D in (1, 15, 16, 17, 32, 33, 512, 8191):
        assert l.dpgp_model_scal_count(D) == R.launch_mirror(D, 2, 1, 1, 1)['scal_count']
    assert l.dpgp_model_scal_count(0) == 0 and l.dpgp_model_scal_count(-3) == 0


def test_rejected_shapes_return_before_any_launch(dev):
    """T = 65 and Q = 31 (PREP_MAX_T, DPGP_MAX_Q): the documented negative return codes."""
    l = _lib.lib()
    one = torch.zeros(8, dtype=F64, device=dev).data_ptr()
    for T, Q, rc in ((65, 2, -2), (2, 31, -3)):
        assert l.dpgp_model_prepare(3, T, Q, 2, 0, 1, *[one] * 8, 1.0, 1.0, 1, *[one] * 6, None) == rc
        assert l.dpgp_model_prepare_t(3, T, Q, 2, 0, 1, *[one] * 8, 1.0, 1.0, 1, *[one] * 4, None) == rc
        assert l.dpgp_model_backward(3, T, Q, 2, 2, 0, 1, 3, *[one] * 10, 1.0, 1.0, 1, *[one] * 15, None) == rc
        assert l.dpgp_model_backward_t(3, T, Q, 2, 2, 0, 1, 3, *[one] * 10, 1.0, 1.0, 1, *[one] * 16, None) == rc
