"""The ragged batched Jacobi on the MI355X: xps_jacobi_sweeps_batched_f64 against one
xps_jacobi_sweeps_f64 call per matrix bit for bit, the freeze protocol, and everything built on it -- eigh_psd_batched on mixed
sizes, pca.fit_many, fit_folds and SVCSearchCV(batch_pca=True) above 128 rows / channels -- against the one-at-a-time route of
the same process, exactly.  Inputs are shifted random PSD matrices from seeded generators."""
import functools
import sys
from collections import Counter

import numpy as np
import pytest
import torch
from sklearn.model_selection import KFold
from sklearn.pipeline import make_pipeline

pytestmark = pytest.mark.gpu

ENTRY, SINGLE = 'xps_jacobi_sweeps_batched_f64', 'xps_jacobi_sweeps_f64'
NAN = float('nan')


def LA():
    from cross_patient_speech_decoding_amd.alignment import _linalg
    return _linalg


def stream():
    from cross_patient_speech_decoding_amd import _dev
    return _dev.stream()


def psd(n, seed, scale=1.0):
    """B B^T * scale + 0.5 I with B (n, n // 2): the construction of test_jacobi_single_workgroup_kernel."""
    Bm = np.random.default_rng(seed).standard_normal((n, max(n // 2, 1)))
    return Bm @ Bm.T * scale + 0.5 * np.eye(n)


# ================================================================================================ 1. the entry
# (m, n, ldw): nb = 6 (33, 40: odd and even block counts before padding; 33 has a phantom block), 18 (130, 136, 137), 26 (201)
# and 8 (300 x 64 with padded columns) -- the smallest and a large nb in one launch sequence
SHAPES = [(33, 33, 33), (40, 40, 40), (130, 130, 130), (136, 136, 136), (137, 137, 137), (201, 201, 201), (300, 64, 307)]


@functools.lru_cache(maxsize=None)
def entry_inputs():
    """Host matrices, column-major with NaN in the padding between columns: [(n, ldw) ndarray] (read-only, shared)."""
    rng = np.random.default_rng(42)
    mats = []
    for i, (m, n, ldw) in enumerate(SHAPES):
        A = psd(n, 100 + i) if m == n else rng.standard_normal((n, m))         # row j = column j
        W = np.full((n, ldw), NAN)
        W[:, :m] = A
        W.setflags(write=False)
        mats.append(W)
    return mats


def pack(mats, gap=5):
    """One device buffer with the matrices `gap` NaN doubles apart; returns (buf, offsets)."""
    offs, pos = [], 3
    for W in mats:
        offs.append(pos)
        pos += W.size + gap
    host = np.full(pos, NAN)
    for o, W in zip(offs, mats):
        host[o:o + W.size] = W.reshape(-1)
    return torch.from_numpy(host).cuda(), offs


class Batch:
    """Device state of one batch for the entry: buffer, tables, off / frozen / sweeps_done."""

    def __init__(self, mats, shapes, tol=0.0):
        la = LA()
        self.buf, offs = pack(mats)
        self.shapes, self.offs = shapes, offs
        b = len(mats)
        self.w_off = np.asarray(offs, dtype=np.int64)
        self.ldw = np.asarray([s[2] for s in shapes], dtype=np.int64)
        self.m = np.asarray([s[0] for s in shapes], dtype=np.int32)
        self.n = np.asarray([s[1] for s in shapes], dtype=np.int32)
        self.tol = torch.from_numpy(np.broadcast_to(np.asarray(tol, dtype=np.float64), (b,)).copy()).cuda()
        self.off = torch.full((b,), 7.0, dtype=torch.float64, device='cuda')
        self.frozen = torch.zeros(b, dtype=torch.int32, device='cuda')
        self.done = torch.zeros(b, dtype=torch.int32, device='cuda')
        self.nb = int(la.lib().xps_jacobi_sweeps_batched_f64_workspace(b))
        self.ws = torch.empty(self.nb // 8 + 1, dtype=torch.int64, device='cuda')

    def run(self, sweeps, check):
        from cross_patient_speech_decoding_amd._lib import call
        try:
            call(ENTRY, self.buf.data_ptr(), self.buf.numel(), self.w_off.ctypes.data, self.ldw.ctypes.data, self.m.ctypes.data,
                 self.n.ctypes.data, len(self.shapes), sweeps, check, self.tol.data_ptr(), self.off.data_ptr(),
                 self.frozen.data_ptr(), self.done.data_ptr(), self.ws.data_ptr(), self.nb, stream())
        finally:
            torch.cuda.synchronize()

    def matrices(self):
        host = self.buf.cpu().numpy()
        return [host[o:o + n * ld].reshape(n, ld) for o, (m, n, ld) in zip(self.offs, self.shapes)]

    def outside(self):
        """Every double of the buffer that belongs to no matrix element: must stay NaN."""
        host = self.buf.cpu().numpy().copy()
        for o, (m, n, ld) in zip(self.offs, self.shapes):
            host[o:o + n * ld].reshape(n, ld)[:, :m] = NAN
        return host


class Single:
    """The same matrix through xps_jacobi_sweeps_f64, alone."""

    def __init__(self, W, shape):
        self.W, self.shape = torch.from_numpy(np.array(W)).cuda(), shape
        self.off = torch.full((1,), 7.0, dtype=torch.float64, device='cuda')

    def run(self, sweeps):
        from cross_patient_speech_decoding_amd._lib import call
        m, n, ld = self.shape
        try:
            call(SINGLE, self.W.data_ptr(), ld, None, n, m, n, sweeps, self.off.data_ptr(), None, 0, stream())
        finally:
            torch.cuda.synchronize()


def same_bits(a, b):
    np.testing.assert_array_equal(np.ascontiguousarray(a).view(np.int64), np.ascontiguousarray(b).view(np.int64))


@pytest.mark.parametrize('which', ['all seven', 'one'])
def test_batched_entry_equals_one_single_call_per_matrix_bit_for_bit(which):
    mats, shapes = entry_inputs(), SHAPES
    if which == 'one':
        mats, shapes = mats[4:5], shapes[4:5]
    batch = Batch(mats, shapes)
    singles = [Single(W, s) for W, s in zip(mats, shapes)]
    for sweeps in (5, 1):
        batch.run(sweeps, 0)
        got, offs = batch.matrices(), batch.off.cpu().numpy()
        assert np.isnan(batch.outside()).all()                            # padding and gaps: neither read into a result nor written
        for b, (s, (m, n, ld)) in enumerate(zip(singles, shapes)):
            s.run(sweeps)
            same_bits(got[b][:, :m], s.W.cpu().numpy()[:, :m])
            same_bits(offs[b:b + 1], s.off.cpu().numpy())
            assert np.isfinite(got[b][:, :m]).all() and 0.0 <= offs[b] <= 1.0
    assert int(batch.frozen.sum()) == 0 and int(batch.done.sum()) == 0     # check == 0: no freeze, no count


def jacobi_alone_sweeps(monkeypatch, C):
    """Sweeps LA._jacobi runs on the square matrix C alone (5 for the first call, 1 for every further one), and the result."""
    la = LA()
    calls = []
    real = la.call
    monkeypatch.setattr(la, 'call', lambda name, *a: (calls.append((name, a[6])), real(name, *a))[1])
    W = torch.from_numpy(np.array(C)).cuda()
    la._jacobi(W, C.shape[0], C.shape[0], want_v=False)
    monkeypatch.setattr(la, 'call', real)
    assert calls and all(name == SINGLE for name, _ in calls)
    return sum(k for _, k in calls), W.cpu().numpy()


def test_freeze_protocol_and_sweep_counts(monkeypatch):
    la = LA()
    sizes = [130, 137, 160, 201, 136]
    Cs = [psd(n, 7 + n) for n in sizes]
    diag = np.diag(np.linspace(1.0, 2.0, 64))
    alone = [jacobi_alone_sweeps(monkeypatch, C) for C in Cs]
    mats = [np.array(C) for C in Cs] + [diag, np.array(Cs[1])]
    shapes = [(n, n, n) for n in sizes] + [(64, 64, 64), (137, 137, 137)]
    tol = [la._jacobi_tol(m, n) for m, n, _ in shapes]
    batch = Batch(mats, shapes, tol)
    batch.frozen[6] = 1                                                    # the last matrix is marked frozen before the first call
    batch.run(5, 1)
    frozen = batch.frozen.cpu().numpy()
    assert frozen[5] == 1 and frozen[6] == 1                               # the diagonal matrix freezes at the first checked call
    assert batch.off.cpu().numpy()[5] == 0.0 and batch.off.cpu().numpy()[6] == 7.0
    same_bits(batch.matrices()[5], diag)
    calls = 1
    while not batch.frozen.cpu().numpy().all():
        batch.run(1, 1)
        calls += 1
        assert calls <= 40
    done = batch.done.cpu().numpy()
    got = batch.matrices()
    print('sweeps per matrix', dict(zip(sizes, done[:5])), 'single-sweep calls', calls - 1)
    for b, (sweeps, W) in enumerate(alone):
        assert done[b] == sweeps, (sizes[b], done[b], sweeps)              # stopped where _jacobi stops it alone
        same_bits(got[b], W)
    assert done[5] == 5 and done[6] == 0
    same_bits(got[6], Cs[1])                                               # frozen from the start: bit-unchanged
    before = batch.buf.clone()
    batch.run(3, 1)                                                        # every matrix frozen: a call changes nothing
    assert torch.equal(before.view(torch.int64), batch.buf.view(torch.int64))
    np.testing.assert_array_equal(batch.done.cpu().numpy(), done)
    # jacobi_ragged: the same stops, found with a number of downloads that does not depend on the batch
    views, ragged_done = la.jacobi_ragged([torch.from_numpy(np.array(C)).cuda() for C in Cs])
    np.testing.assert_array_equal(ragged_done, [s for s, _ in alone])
    for v, (_, W) in zip(views, alone):
        same_bits(v.cpu().numpy(), W)


# ================================================================================================ 2. eigh_psd_batched
def check_eigs(res, Cs):
    """test_jacobi_single_workgroup_kernel's bars against numpy."""
    for (w, V), C in zip(res, Cs):
        n = C.shape[0]
        np.testing.assert_allclose(w, np.linalg.eigvalsh(C)[::-1], rtol=1e-11)
        np.testing.assert_allclose(V.T @ V, np.eye(n), atol=1e-11)
        np.testing.assert_allclose(V.T @ C @ V, np.diag(w), atol=1e-10 * w[0])


def same_eigs(a, b):
    assert len(a) == len(b)
    for (wa, Va), (wb, Vb) in zip(a, b):
        same_bits(wa, wb)
        same_bits(Va, Vb)


@functools.lru_cache(maxsize=None)
def mixed_list():
    Cs = [psd(n, 11 * i + n, 1.0 + i) for i, n in enumerate([130, 24, 137, 137, 24, 201])]
    for C in Cs:
        C.setflags(write=False)
    return Cs


def test_eigh_psd_batched_mixed_sizes_equals_one_at_a_time_and_numpy():
    la = LA()
    Cs = mixed_list()
    res = la.eigh_psd_batched(Cs)
    assert [len(w) for w, _ in res] == [130, 24, 137, 137, 24, 201]        # input order
    same_eigs(res, la.eigh_psd_batched(Cs, one_at_a_time=True))
    big = [0, 2, 3, 5]                                                     # beyond the one-workgroup kernel: eigh_psd's own bits too
    same_eigs([res[i] for i in big], [la.eigh_psd(torch.from_numpy(np.array(Cs[i])).cuda()) for i in big])
    check_eigs(res, Cs)
    same_eigs(res, la.eigh_psd_batched(Cs))                                # determinism: two runs, the same bits
    dev = [torch.from_numpy(np.array(C)).cuda() for C in Cs]               # device tensors in the list
    res_d = la.eigh_psd_batched(dev)
    same_eigs(res_d, la.eigh_psd_batched(dev, one_at_a_time=True))
    same_eigs([res_d[i] for i in big], [res[i] for i in big])
    stack = np.stack([psd(136, 900 + i, 1.0 + 0.5 * i) for i in range(4)])
    res = la.eigh_psd_batched(stack)
    same_eigs(res, la.eigh_psd_batched(stack, one_at_a_time=True))
    check_eigs(res, stack)
    same_eigs(la.eigh_psd_batched(stack, well_conditioned=True), la.eigh_psd_batched(stack, True, one_at_a_time=True))


def test_small_ndarrays_in_a_list_are_shifted_as_an_ndarray_stack_is():
    """A list of ndarrays within the one-workgroup kernel -- of one size, or beside other sizes -- gives the bits of the same
    matrices handed over as one (batch, n, n) ndarray (the shift is taken on the host in both): what build_plan_pca relies on."""
    la = LA()
    for n in (40, 97):
        Cs = [psd(n, 300 + 7 * i + n, 1.0 + i) for i in range(3)]
        ref = la.eigh_psd_batched(np.stack(Cs))
        same_eigs(la.eigh_psd_batched(Cs), ref)
        mixed = la.eigh_psd_batched([Cs[0], Cs[1], mixed_list()[2], Cs[2]])
        same_eigs([mixed[0], mixed[1], mixed[3]], ref)
        check_eigs(ref, Cs)


def test_a_rank_deficient_matrix_in_the_batch_takes_the_fallback():
    la = LA()
    Bm = np.random.default_rng(130).standard_normal((130, 65))
    low = Bm @ Bm.T                                                        # rank 65: _eig_from_w rejects it, V must be accumulated
    Cs = [mixed_list()[2], low, mixed_list()[5]]
    res = la.eigh_psd_batched(Cs)
    same_eigs(res, la.eigh_psd_batched(Cs, one_at_a_time=True))
    check_eigs([res[0], res[2]], [Cs[0], Cs[2]])
    w, V = res[1]
    wr = np.linalg.eigvalsh(low)[::-1]
    np.testing.assert_allclose(w, wr, atol=1e-10 * wr[0])                  # (the bars of the rank-deficient case of that test)
    np.testing.assert_allclose(V.T @ V, np.eye(130), atol=1e-12)
    np.testing.assert_allclose(V.T @ low @ V, np.diag(w), atol=1e-10 * wr[0])


def count_calls(monkeypatch):
    from cross_patient_speech_decoding_amd import _lib
    counts = Counter()
    real = _lib.call

    def counting(name, *args):
        counts[name] += 1
        return real(name, *args)
    for mod in list(sys.modules.values()):                                # every module that bound `call` by name
        if getattr(mod, '__name__', '').startswith('cross_patient_speech_decoding_amd') and getattr(mod, 'call', None) is real:
            monkeypatch.setattr(mod, 'call', counting)
    return counts


def test_call_counts_do_not_grow_with_the_batch(monkeypatch):
    la = LA()
    counts = count_calls(monkeypatch)
    C = mixed_list()[2]
    one = la.eigh_psd_batched([C])
    n_one = counts[ENTRY]
    assert n_one >= 2 and counts[SINGLE] == 0, dict(counts)
    counts.clear()
    eight = la.eigh_psd_batched([C] * 8)
    assert counts[ENTRY] == n_one and counts[SINGLE] == 0, dict(counts)
    for r in eight:
        same_eigs([r], one)
    counts.clear()
    la.eigh_psd_batched(mixed_list())
    assert counts[SINGLE] == 0 and counts['xps_jacobi_small_f64'] == 1, dict(counts)      # the two 24 x 24: one launch


# ================================================================================================ 3. the callers
def one_at_a_time(monkeypatch):
    la = LA()
    real = la.eigh_psd_batched
    monkeypatch.setattr(la, 'eigh_psd_batched', lambda Cs, well_conditioned=False, one_at_a_time=False: real(Cs, well_conditioned, True))
    return real


def test_fit_many_equals_separate_fits_exactly(monkeypatch):
    import cross_patient_speech_decoding_amd.alignment as A
    rng = np.random.default_rng(5)
    Xs = [(rng.standard_normal((300, 8)) @ rng.standard_normal((8, d)) + 0.3 * rng.standard_normal((300, d))).astype(np.float32)
          for d in (24, 130, 140)]
    counts = count_calls(monkeypatch)
    many = A.fit_many(Xs, n_components=0.9)
    assert counts[SINGLE] == 0 and counts[ENTRY] >= 1, dict(counts)
    for m, x in zip(many, Xs):
        ref = A.PCA(n_components=0.9).fit(x)
        assert isinstance(m, A.PCA) and m.n_components_ == ref.n_components_ and m.n_features_in_ == ref.n_features_in_
        assert 1 <= m.n_components_ < x.shape[1] and m.n_samples_ == ref.n_samples_
        for name in ('mean_', 'components_', 'explained_variance_', 'explained_variance_ratio_', 'singular_values_'):
            same_bits(getattr(m, name), getattr(ref, name))
        same_bits(m.transform(x), ref.transform(x))
    assert A.fit_many([], n_components=3) == []
    with pytest.raises(ValueError, match='covariance'):
        A.fit_many(Xs, solver='gram')


def test_reduce_each_through_fit_many_equals_the_loop_exactly():
    import cross_patient_speech_decoding_amd.alignment as A
    from cross_patient_speech_decoding_amd.decoders.cross_pt_decoders import crossPtDecoder_sepDimRed
    from cross_patient_speech_decoding_amd.utils.synthetic import make_patient

    class LoopPCA(A.PCA):                                                  # not `alignment.PCA` itself: _reduce_each keeps its loop
        pass
    X, _ = make_patient(0, 30, T=10, C=24, n_cond=6, k=4)
    pool = [make_patient(p, 30 + 3 * p, T=10, C=c, n_cond=6, k=4) for p, c in ((1, 140), (2, 24))]
    data = [(x, y[:, 0], y[:, 0]) for x, y in pool]
    many = crossPtDecoder_sepDimRed(data, None, dim_red=A.PCA, n_comp=0.8)
    loop = crossPtDecoder_sepDimRed(data, None, dim_red=LoopPCA, n_comp=0.8)
    (tar_m, out_m), (tar_l, out_l) = many._reduce_each(X), loop._reduce_each(X)
    assert isinstance(many.tar_dr, A.PCA) and tar_m.shape[:2] == (30, 10) and [o.shape[0] for o in out_m] == [33, 36]
    for a, b in zip([tar_m] + out_m, [tar_l] + out_l):
        assert a.dtype == b.dtype and a.shape == b.shape
        same_bits(a, b)
    for name in ('mean_', 'components_', 'explained_variance_'):
        same_bits(getattr(many.tar_dr, name), getattr(loop.tar_dr, name))
    Xt = X[:5] * 1.01
    same_bits(many.tar_dr.transform(Xt.reshape(-1, 24)), loop.tar_dr.transform(Xt.reshape(-1, 24)))


def test_fit_folds_above_128_channels_is_the_one_at_a_time_fit_bit_for_bit(monkeypatch):
    import cross_patient_speech_decoding_amd.alignment as A
    from cross_patient_speech_decoding_amd.utils.synthetic import make_patient
    T = 20
    pats = [make_patient(p, 40 + 3 * p, T=T, C=c, n_cond=10, k=6, noise=0.5) for p, c in enumerate([130, 140, 24])]
    X, y = pats[0]
    pool = [(x, yy, yy) for x, yy in pats[1:]]
    splits = list(KFold(4, shuffle=True, random_state=0).split(X))
    counts = count_calls(monkeypatch)
    fa = A.fit_folds(X, y, pool, splits)
    assert counts[SINGLE] == 0 and counts[ENTRY] >= 2, dict(counts)        # the fold covariances and the 140-channel patient
    one_at_a_time(monkeypatch)
    counts.clear()
    ref = A.fit_folds(X, y, pool, splits)
    assert counts[SINGLE] > 0 and counts[ENTRY] == 0, dict(counts)         # (the comparator did take the other route)
    assert fa.fallbacks_ == ref.fallbacks_ and fa.n_components_ == ref.n_components_
    for f in range(len(splits)):
        assert torch.equal(fa.train_pool(f), ref.train_pool(f))
        for name in ('pca_mean_', 'pca_components_', 'explained_variance_', 'explained_variance_ratio_all_'):
            same_bits(getattr(fa, name)[f], getattr(ref, name)[f])
        for p in range(len(pool)):
            for name in ('M_a_', 'M_b_', 'canon_corrs_'):
                same_bits(getattr(fa, name)[f][p], getattr(ref, name)[f][p])
            assert torch.equal(fa.maps_[f][p], ref.maps_[f][p])


def test_svc_search_with_batched_pca_above_128_rows(monkeypatch):
    import cross_patient_speech_decoding_amd.alignment as A
    from cross_patient_speech_decoding_amd.decoders import SVC, SVCSearchCV
    from cross_patient_speech_decoding_amd.decomposition import DimRedReshape
    from cross_patient_speech_decoding_amd.utils.synthetic import make_patient
    X, y_full = make_patient(3, 203, T=12, C=20, n_cond=12, k=4)           # 203 rows of 240 features
    y = y_full[:, 0]
    cv = KFold(3)
    assert sorted(len(tr) for tr, _ in cv.split(X)) == [135, 135, 136]
    NC = 'dimredreshape__n_components'
    grid = {NC: [0.5, 0.9, 5], 'svc__C': [1, 10], 'svc__gamma': ['scale']}
    pipe = lambda: make_pipeline(DimRedReshape(A.GramPCA), SVC(kernel='rbf', class_weight='balanced', tol=1e-6))
    counts = count_calls(monkeypatch)
    fused = SVCSearchCV(pipe(), grid, cv=cv, refit=False, batch_pca=True).fit(X, y)
    assert counts[SINGLE] == 0 and counts[ENTRY] >= 2, dict(counts)
    for entry in ('xps_gram_center_folds_f64', 'xps_apply_grouped_f64', 'xps_prefix_kernels_f64', 'xps_svm_smo_multi_f64',
                  'xps_svm_cv_score_f64', 'xps_colsum_f64'):
        assert counts[entry] == 1, (entry, dict(counts))
    assert counts['xps_dgemm_small'] + counts['xps_dgemm_splitk'] == 1, dict(counts)
    assert fused.cv_confusion_.shape[:2] == (6, 3)
    one_at_a_time(monkeypatch)
    counts.clear()
    ref = SVCSearchCV(pipe(), grid, cv=cv, refit=False, batch_pca=True).fit(X, y)
    assert counts[SINGLE] > 0 and counts[ENTRY] == 0, dict(counts)
    np.testing.assert_array_equal(fused.cv_confusion_, ref.cv_confusion_)
    np.testing.assert_array_equal(fused.pca_n_components_, ref.pca_n_components_)
    assert sorted(fused.cv_results_) == sorted(ref.cv_results_)
    for key, val in fused.cv_results_.items():
        if key == 'params':
            assert val == ref.cv_results_[key]
        elif key.startswith('param_'):
            assert list(val) == list(ref.cv_results_[key])
        else:
            same_bits(np.asarray(val, dtype=np.float64), np.asarray(ref.cv_results_[key], dtype=np.float64))
    for (_, a), (_, b) in zip(fused.cv_test_predictions_, ref.cv_test_predictions_):
        np.testing.assert_array_equal(a, b)
