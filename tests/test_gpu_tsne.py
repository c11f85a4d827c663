"""manifold.TSNE on the MI355X: the bit-for-bit promises of the batched form (a data set alone, first / last in a batch, on two
streams, twice), the frozen problem, the launch and synchronisation counts, the end-to-end fit of n130_D100 against sklearn's own
spread, ``kl_divergence_`` against the restatement at the device's own embedding, and the composition with cluster_scores.

Chaos makes a final embedding incomparable pointwise (tests/test_gpu_tsne_kernels.py holds the first ten iterations), so the
end-to-end reference is the spread of sklearn's exact t-SNE over four inits that differ by 1e-12 relative."""
import sys

import numpy as np
import pytest
import torch
from sklearn.manifold import TSNE as SkTSNE, trustworthiness

import cluster_ref as CR
import tsne_ref as TR

pytestmark = pytest.mark.gpu

CASES = TR.cases()
BATCH = ['n5_D3', 'n65_D17_f32', 'n130_D100']
_alone = {}


def MF():
    from cross_patient_speech_decoding_amd import manifold
    return manifold


def LA():
    from cross_patient_speech_decoding_amd.alignment import _linalg
    return _linalg


def bits(a):
    return np.ascontiguousarray(np.asarray(a, dtype=np.float64)).view(np.int64)


def init_of(name):
    return TR.random_init(len(CASES[name][0]), 2, 11)


def make(perplexity=2.0, **kw):
    return MF().TSNE(perplexity=perplexity, **kw)


def alone(name):
    """(embedding, kl, n_iter, sigma) of a batch member fitted alone with perplexity 2; computed once and left unchanged."""
    if name not in _alone:
        ts = make(init=init_of(name))
        Y = ts.fit_transform(CASES[name][0])
        _alone[name] = (Y.copy(), ts.kl_divergence_, ts.n_iter_, ts.sigma_.copy())
    return _alone[name]


def same_as_alone(ts, i, name):
    Y, kl, it, sigma = alone(name)
    assert np.array_equal(bits(ts.embeddings_[i]), bits(Y)), f'{name}: embedding differs'
    assert bits(ts.kl_divergences_[i]) == bits(kl) and ts.n_iters_[i] == it
    assert np.array_equal(bits(ts.sigmas_[i]), bits(sigma))


# ------------------------------------------------------------------------------------------------ bit-for-bit
def test_a_data_set_gives_the_same_bits_alone_first_and_last_in_a_batch_and_on_two_streams():
    for order in (BATCH, BATCH[::-1]):
        ts = make()
        out = ts.fit_transform_many([CASES[n][0] for n in order], inits=[init_of(n) for n in order])
        assert len(out) == 3 and all(y.dtype == np.float64 and y.shape == (len(CASES[n][0]), 2) for y, n in zip(out, order))
        for i, name in enumerate(order):
            same_as_alone(ts, i, name)
    side = torch.cuda.Stream()
    with torch.cuda.stream(side):
        ts = make(init=init_of('n65_D17_f32'))
        ts.fit_transform(CASES['n65_D17_f32'][0])
    side.synchronize()
    ts.embeddings_ = [ts.embedding_]
    same_as_alone(ts, 0, 'n65_D17_f32')


def test_two_fits_give_the_same_bits_and_the_fitted_attributes_are_sklearns():
    name = 'n130_D100'
    X = CASES[name][0]
    ts = make(init=init_of(name))
    Y = ts.fit(X).embedding_
    Y_first, kl, it, sigma = alone(name)
    assert np.array_equal(bits(Y), bits(Y_first)) and bits(ts.kl_divergence_) == bits(kl)
    assert Y.shape == (130, 2) and Y.dtype == np.float64 and np.isfinite(Y).all()
    assert ts.n_iter_ == it == 999 and ts.n_features_in_ == 100 and ts.learning_rate_ == 50.0
    assert ts.sigma_.shape == (130,) and (ts.sigma_ > 0).all() and np.isfinite(ts.kl_divergence_) and ts.kl_divergence_ > 0


def test_random_init_draws_run_through_the_batch_and_pca_init_and_one_component_and_precomputed_run():
    names = ['n5_D3', 'n65_D17_f32']
    Xs = [CASES[n][0] for n in names]
    ts = make(init='random', random_state=3, max_iter=250)
    ts.fit_transform_many(Xs)
    rng = np.random.RandomState(3)
    draws = [(1e-4 * rng.standard_normal((len(X), 2)).astype(np.float32)).astype(np.float64) for X in Xs]
    again = make(max_iter=250)
    again.fit_transform_many(Xs, inits=draws)
    for a, b in zip(ts.embeddings_, again.embeddings_):
        assert np.array_equal(bits(a), bits(b))
    X = CASES['n130_D100'][0]
    for kw in (dict(init='pca'), dict(init='pca', n_components=1), dict(init='random', random_state=0, metric='precomputed')):
        ts = make(perplexity=30.0, max_iter=250, **kw)
        data = np.sqrt(np.asarray(CR.sq_dists(X), dtype=np.float64)) if kw.get('metric') else torch.from_numpy(X.astype(np.float32)).cuda()
        Y = ts.fit_transform(data)
        assert Y.shape == (130, kw.get('n_components', 2)) and np.isfinite(Y).all() and ts.n_iter_ == 249 and ts.kl_divergence_ > 0


# ------------------------------------------------------------------------------------------------ the frozen problem
def test_a_frozen_problem_returns_its_init_and_sklearns_n_iter_while_its_neighbour_runs_on():
    X, perp = CASES['n64_D10']
    const = np.full((64, 2), 0.25)
    sk = SkTSNE(method='exact', init=const.copy(), perplexity=2.0).fit(X)
    ts = make()
    ts.fit_transform_many([X, CASES['n130_D100'][0]], inits=[const, init_of('n130_D100')])
    assert ts.n_iters_[0] == sk.n_iter_ == 99
    assert np.array_equal(bits(ts.embeddings_[0]), bits(const))
    same_as_alone(ts, 1, 'n130_D100')
    assert ts.n_iters_[1] == 999


# ------------------------------------------------------------------------------------------------ launches and synchronisations
def count_calls(monkeypatch):
    from collections import Counter
    from cross_patient_speech_decoding_amd import _lib
    from cross_patient_speech_decoding_amd.manifold import tsne
    counts, launches, real, real_dl = Counter(), [], _lib.call, tsne._download

    def counting(name, *args):
        counts[name] += 1
        if name == 'xps_tsne_descent_f64':
            launches.append(args[4])
        return real(name, *args)

    def download(parts):
        counts['download'] += 1
        return real_dl(parts)
    for mod in list(sys.modules.values()):                               # every module that bound `call` by name
        if getattr(mod, '__name__', '').startswith('cross_patient_speech_decoding_amd') and getattr(mod, 'call', None) is real:
            monkeypatch.setattr(mod, 'call', counting)
    monkeypatch.setattr(tsne, '_download', download)
    return counts, launches


@pytest.mark.parametrize('batch', [1, 3])
def test_a_fit_costs_one_launch_per_iteration_and_two_synchronisations_whatever_the_batch(monkeypatch, batch):
    names = BATCH[:batch]
    max_iter = 300
    counts, launches = count_calls(monkeypatch)
    ts = make(max_iter=max_iter)
    ts.fit_transform_many([CASES[n][0] for n in names], inits=[init_of(n) for n in names])
    assert counts.pop('xps_colsum_f64') == batch                         # the column mean of each data set, for the centring
    assert dict(counts) == {'xps_gram_grouped_f64': 1, 'xps_tsne_sqdist_f32': 1, 'xps_tsne_affinities_f64': 1,
                            'xps_tsne_descent_f64': 2, 'download': 2}
    assert launches == [250, max_iter - 250]                             # each call adds one priming launch: max_iter + 2 in all
    assert ts.n_iters_ == [max_iter - 1] * batch


# ------------------------------------------------------------------------------------------------ end to end
def pca_init(X):
    Xc = X - X.mean(axis=0)
    _, _, Vt = np.linalg.svd(Xc, full_matrices=False)
    Y = (Xc @ Vt[:2].T).astype(np.float32)
    return (Y / np.std(Y[:, 0]) * 1e-4).astype(np.float64)


def test_n130_D100_with_default_arguments_lies_in_sklearns_own_spread():
    X, _ = CASES['n130_D100']
    Y0 = pca_init(X)
    kls, trusts = [], []
    for r in range(4):
        g = np.random.default_rng(100 + r).standard_normal(Y0.shape)
        sk = SkTSNE(method='exact', init=Y0 * (1 + 1e-12 * g))
        trusts.append(trustworthiness(X, sk.fit_transform(X)))
        kls.append(sk.kl_divergence_)
    ts = MF().TSNE(init=Y0)
    Y = ts.fit_transform(X)
    w, tw = max(kls) - min(kls), max(trusts) - min(trusts)
    trust = trustworthiness(X, Y)
    print(f'sklearn KL {min(kls):.6f} .. {max(kls):.6f}, trustworthiness {min(trusts):.6f} .. {max(trusts):.6f}; '
          f'device KL {ts.kl_divergence_:.6f}, trustworthiness {trust:.6f}, n_iter {ts.n_iter_}')
    assert min(kls) - w <= ts.kl_divergence_ <= max(kls) + w
    assert trust >= min(trusts) - tw


def test_kl_divergence_is_the_restatements_error_at_the_devices_own_embedding():
    la = LA()
    X, _ = CASES['n130_D100']
    n, max_iter = 130, 1000
    Y0 = pca_init(X)
    ts = MF().TSNE(init=Y0)
    ts.fit(X)
    # the same pipeline through the wrappers of the C entry points, stopped one launch short of the fit's last iteration (the
    # prefix is bit-identical): n_iter_ is max_iter - 1, or the check at which the fit stopped
    last = ts.n_iter_
    assert last == max_iter - 1 or (last + 1) % 50 == 0
    dev = la.device()
    Xd = la.to_device(X)
    pr = dict(n=n, nc=2, G=torch.empty(n, n, dtype=la.F64, device=dev), D2=torch.empty(n, n, dtype=torch.float32, device=dev),
              steps=torch.empty(n, dtype=torch.int32, device=dev), state=la.tsne_state(n, dev), lr=ts.learning_rate_, it_begin=0)
    for key, shape in (('C', (n, n)), ('P', (n, n)), ('beta', (n,)), ('rowsum', (n,))):
        pr[key] = torch.empty(*shape, dtype=la.F64, device=dev)
    pr['Y_in'] = pr['Y_out'] = torch.from_numpy(Y0).to(dev)
    keep = [la.gram_grouped([(Xd.to(la.F64) - la.col_mean(Xd), pr['G'])]), la.tsne_sqdist([pr]), la.tsne_affinities([pr], 30.0),
            la.tsne_descent([pr], 250, 250, 0.5, 12.0, 250, 1e-7)]
    torch.cuda.synchronize()
    assert pr['state'][0].item() == 249.0
    pr['it_begin'] = 250
    keep.append(la.tsne_descent([pr], last - 250, max_iter, 0.8, 1.0, 300, 1e-7))
    torch.cuda.synchronize()
    half = (la.TSNE_STATE_HEAD + 15 * n) * ((last - 250) & 1)
    st = pr['state'].cpu().numpy()[half:half + la.TSNE_STATE_HEAD + 15 * n]
    assert st[0] == last and st[4] == 0.0                                # the next iteration is the fit's last; not done
    Y = np.stack([st[8:8 + n], st[8 + n:8 + 2 * n]], axis=1)
    P = pr['P'].cpu().numpy()
    pt = TR.partials(P, Y, True)
    _, _, err = TR.objective(pt, 1.0)
    _, _, derr = TR.objective_bars(pt, TR.partials_bars(P, Y), 1.0)
    print(f'n_iter_ {last}; kl_divergence_ {ts.kl_divergence_:.17g}, restatement {float(err):.17g}, bar {derr:.3e}')
    assert abs(ts.kl_divergence_ - float(err)) <= derr


def test_the_embedding_composes_with_cluster_scores():
    from cross_patient_speech_decoding_amd.alignment import metrics
    X, labels = CR.make_case(130, 100, 9, 24)
    Y = make(perplexity=30.0, max_iter=250, init=pca_init(X)).fit_transform(X)
    a = metrics.cluster_scores(Y, labels, n_shuffles=8, random_state=1)
    b = metrics.cluster_scores(np.array(Y, copy=True), labels, n_shuffles=8, random_state=1)
    for key in ('silhouette_samples_', 'silhouette_', 'silhouette_pos_', 'calinski_harabasz_', 'davies_bouldin_'):
        assert np.array_equal(bits(getattr(a, key)), bits(getattr(b, key)))
    assert np.isfinite(a.silhouette_pos_[0])
