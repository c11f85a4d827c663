"""alignment/metrics.py on the MI355X: the cluster separability scores against the long-double restatement of
tests/cluster_ref.py (and sklearn beside it), the bit-for-bit promises of cluster_scores (set 0 = the single functions, set r =
that permutation alone, any chunking), its p-values and launch counts, and pt_corr / pt_corr_multi against scipy.

The bars come from the data of each case (tests/cluster_ref.py derives them): |delta s| <= 4 (eps + n u) for every silhouette,
a relative 8 (D + n) u kappa for Calinski-Harabasz and Davies-Bouldin.  sklearn works in float64 as well and carries an error
of the same kind on the data as given (not centred), so the device result may differ from it by the sum of the two bars."""
import sys

import numpy as np
import pytest
from scipy import stats
from sklearn import metrics as SK

import cluster_ref as CR

pytestmark = pytest.mark.gpu

U = 2.0 ** -53
SEED = 5
CASES = CR.cases()
SHUFFLES = {'n130_D100_k9': 65, 'n65_D17_k3_f32': 65, 'n64_D6000_k9_f32': 8, 'n12_D5_k4_singleton': 65, 'n40_D8_k5_strings': 65}
_scored = {}


def MT():
    from cross_patient_speech_decoding_amd.alignment import metrics
    return metrics


def bits(a):
    return np.ascontiguousarray(np.asarray(a, dtype=np.float64)).view(np.int64)


def arrays(cs):
    return dict(sil=cs.silhouette_samples_, mean=cs.silhouette_, pos=cs.silhouette_pos_, ch=cs.calinski_harabasz_,
                db=cs.davies_bouldin_)


def same_bits(a, b, what=''):
    for name in a:
        assert np.array_equal(bits(a[name]), bits(b[name])), f'{what}: {name} differs'


def scored(name):
    """cluster_scores of a case with its shuffles, computed once and left unchanged."""
    if name not in _scored:
        X, labels = CASES[name]
        _scored[name] = MT().cluster_scores(X, labels, n_shuffles=SHUFFLES[name], random_state=SEED)
    return _scored[name]


def count_calls(monkeypatch):
    from collections import Counter
    from cross_patient_speech_decoding_amd import _lib
    counts, real = Counter(), _lib.call

    def counting(name, *args):
        counts[name] += 1
        return real(name, *args)
    for mod in list(sys.modules.values()):                               # every module that bound `call` by name
        if getattr(mod, '__name__', '').startswith('cross_patient_speech_decoding_amd') and getattr(mod, 'call', None) is real:
            monkeypatch.setattr(mod, 'call', counting)
    return counts


# ------------------------------------------------------------------------------------------------ parity
@pytest.mark.parametrize('name', sorted(CASES))
def test_scores_stay_within_the_derived_bars_of_the_restatement_and_of_sklearn(name):
    X, labels = CASES[name]
    X64 = X.astype(np.float64)
    R = SHUFFLES[name]
    cs = scored(name)
    sets = [labels] + CR.shuffles(labels, R, SEED)
    assert cs.n_shuffles == R and len(cs.labels_) == R + 1 and all(np.array_equal(a, b) for a, b in zip(cs.labels_, sets))
    assert cs.silhouette_samples_.shape == (R + 1, len(X)) and cs.silhouette_samples_.dtype == np.float64
    for a in (cs.silhouette_, cs.silhouette_pos_, cs.calinski_harabasz_, cs.davies_bouldin_):
        assert a.shape == (R + 1,) and a.dtype == np.float64
    d2 = CR.sq_dists(X64)
    bar, bar_sk = CR.silhouette_bar(X64, d2), CR.silhouette_bar(X64, d2, centre=False)
    used = dict(sil=0.0, ch=0.0, db=0.0)
    for r, y in enumerate(sets):
        s = CR.silhouette_samples(X64, y, d2)
        err = float(np.abs(cs.silhouette_samples_[r] - s).max())
        used['sil'] = max(used['sil'], err / bar)
        assert err <= bar, f'set {r}: silhouettes off by {err:.3e}, bar {bar:.3e}'
        assert abs(cs.silhouette_[r] - s.sum() / len(s)) <= bar + len(s) * U
        if (np.abs(s) > bar).all():                                     # the positive ones are the same samples on both sides
            assert abs(cs.silhouette_pos_[r] - CR.positive_mean(s)) <= bar + len(s) * U
        ch_bar, db_bar = CR.dispersion_bars(X64, y)
        ch, db = CR.calinski_harabasz(X64, y), CR.davies_bouldin(X64, y)
        e_ch, e_db = float(abs(cs.calinski_harabasz_[r] - ch) / abs(ch)), float(abs(cs.davies_bouldin_[r] - db) / abs(db))
        used['ch'], used['db'] = max(used['ch'], e_ch / ch_bar), max(used['db'], e_db / db_bar)
        assert e_ch <= ch_bar, f'set {r}: Calinski-Harabasz off by {e_ch:.3e} relative, bar {ch_bar:.3e}'
        assert e_db <= db_bar, f'set {r}: Davies-Bouldin off by {e_db:.3e} relative, bar {db_bar:.3e}'
        if r < 3:                                                       # sklearn beside it, on the float64 copy of the data
            assert np.abs(cs.silhouette_samples_[r] - SK.silhouette_samples(X64.reshape(len(X), -1), y)).max() <= bar + bar_sk
            ch_sk, db_sk = CR.dispersion_bars(X64, y, centre=False)
            assert abs(cs.calinski_harabasz_[r] - SK.calinski_harabasz_score(X64, y)) <= (ch_bar + ch_sk) * abs(ch)
            assert abs(cs.davies_bouldin_[r] - SK.davies_bouldin_score(X64, y)) <= ((db_bar + db_sk) * abs(db)
                                                                                   + CR.sklearn_singleton_slack(X64, y))
    print(f'{name}: largest fraction of the bar: silhouettes {used["sil"]:.2e}, Calinski-Harabasz {used["ch"]:.2e}, '
          f'Davies-Bouldin {used["db"]:.2e}')


@pytest.mark.parametrize('name', sorted(CASES))
def test_set_0_is_the_single_functions_and_set_r_is_that_permutation_alone(name):
    import torch
    mt = MT()
    X, labels = CASES[name]
    cs = scored(name)
    got = arrays(cs)
    single = dict(sil=mt.silhouette_samples(X, labels), mean=mt.silhouette_score(X, labels), pos=mt.silhouette_scorer(X, labels),
                  ch=mt.calinski_harabasz_score(X, labels), db=mt.davies_bouldin_score(X, labels))
    assert single['sil'].dtype == np.float64 and single['sil'].shape == (len(X),)
    assert all(isinstance(single[s], np.float64) for s in ('mean', 'pos', 'ch', 'db'))
    same_bits(single, {k: v[0] for k, v in got.items()}, 'set 0')
    for r in sorted({1, SHUFFLES[name] // 2, SHUFFLES[name]}):
        alone = arrays(mt.cluster_scores(X, cs.labels_[r]))
        same_bits({k: v[0] for k, v in alone.items()}, {k: v[r] for k, v in got.items()}, f'set {r}')
    on_device = arrays(mt.cluster_scores(torch.from_numpy(X).cuda(), labels))            # a device tensor is taken as it is
    same_bits({k: v[0] for k, v in on_device.items()}, {k: v[0] for k, v in got.items()}, 'device input')


@pytest.mark.parametrize('R', (0, 1, 65))
def test_shuffles_chunks_p_values_and_launch_counts(R, monkeypatch):
    mt = MT()
    X, labels = CASES['n65_D17_k3_f32']
    n, k = len(X), 3
    all_shuffles = arrays(scored('n65_D17_k3_f32'))                       # (before the calls are counted)
    counts = count_calls(monkeypatch)
    whole = mt.cluster_scores(X, labels, n_shuffles=R, random_state=SEED)
    per_chunk = dict(counts)
    assert per_chunk.pop('xps_gram_grouped_f64') == 1 and per_chunk.pop('xps_colsum_f64') == 1
    assert per_chunk == {'xps_label_row_sums_f64': 2, 'xps_silhouette_from_sums_f64': 1, 'xps_label_col_sums_f64': 3,
                         'xps_centroid_dist_from_sums_f64': 1}                          # whatever R is
    same_bits(arrays(whole), {k_: v[:R + 1] for k_, v in all_shuffles.items()}, 'fewer shuffles, same draws')
    for chunks, max_bytes in ((R + 1, 1), (min(2, R + 1), mt.bytes_per_set(n, k) * -(-(R + 1) // 2)), (1, 2 ** 28)):
        counts.clear()
        cut = mt.cluster_scores(X, labels, n_shuffles=R, random_state=SEED, max_bytes=max_bytes)
        assert counts['xps_gram_grouped_f64'] == 1 and counts['xps_silhouette_from_sums_f64'] == chunks
        assert counts['xps_label_row_sums_f64'] == 2 * chunks and counts['xps_label_col_sums_f64'] == 3 * chunks
        same_bits(arrays(cut), arrays(whole), f'{chunks} chunks')
    # random_state=None draws from numpy's global generator: np.random.seed(s) reproduces the notebooks' shuffle
    np.random.seed(3)
    glob = mt.cluster_scores(X, labels, n_shuffles=R)
    np.random.seed(3)
    for r in range(1, R + 1):
        assert np.array_equal(glob.labels_[r], np.random.permutation(labels))
    if R:
        same_bits({k_: v[0] for k_, v in arrays(mt.cluster_scores(X, glob.labels_[R])).items()},
                  {k_: v[R] for k_, v in arrays(glob).items()}, 'the global generator')
    # the p-values are the host formula on the function's own arrays
    assert sorted(whole.p_value_) == ['calinski_harabasz', 'davies_bouldin', 'silhouette', 'silhouette_pos']
    for key, arr, smaller in (('silhouette', whole.silhouette_, False), ('silhouette_pos', whole.silhouette_pos_, False),
                              ('calinski_harabasz', whole.calinski_harabasz_, False), ('davies_bouldin', whole.davies_bouldin_, True)):
        hits = sum(1 for v in arr[1:R + 1] if (v <= arr[0] if smaller else v >= arr[0]))
        assert whole.p_value_[key] == (1 + hits) / (1 + R)
    if R == 65:
        assert whole.p_value_['silhouette'] == 1 / 66 and whole.p_value_['davies_bouldin'] == 1 / 66       # a real structure


def test_extra_label_sets_have_their_own_classes_and_stay_out_of_the_null():
    mt = MT()
    X, labels = CASES['n130_D100_k9']
    artic = np.array(['lab', 'lab', 'cor', 'cor', 'dor', 'dor', 'dor', 'vow', 'vow'])[labels]          # 4 classes beside 9
    wide = np.arange(len(X)) % 64                                                                        # 64 classes
    cs = mt.cluster_scores(X, labels, n_shuffles=3, random_state=SEED, label_sets=[artic, wide])
    assert cs.silhouette_samples_.shape == (6, len(X)) and np.array_equal(cs.labels_[4], artic)
    same_bits({k: v[:4] for k, v in arrays(cs).items()}, {k: v[:4] for k, v in arrays(scored('n130_D100_k9')).items()}, 'the null')
    assert cs.p_value_ == mt.cluster_scores(X, labels, n_shuffles=3, random_state=SEED).p_value_
    for r, y in ((4, artic), (5, wide)):
        same_bits({k: v[0] for k, v in arrays(mt.cluster_scores(X, y)).items()}, {k: v[r] for k, v in arrays(cs).items()}, f'extra {r}')
    d2 = CR.sq_dists(X)
    assert np.abs(cs.silhouette_samples_[4] - CR.silhouette_samples(X, artic, d2)).max() <= CR.silhouette_bar(X, d2)
    ch_bar, db_bar = CR.dispersion_bars(X, artic)
    ch, db = CR.calinski_harabasz(X, artic), CR.davies_bouldin(X, artic)
    assert abs(cs.calinski_harabasz_[4] - ch) <= ch_bar * abs(ch) and abs(cs.davies_bouldin_[4] - db) <= db_bar * abs(db)
    seq = np.stack([labels, labels[::-1] % 2], axis=1)                                                   # 2-D sequence labels
    same_bits(arrays(mt.cluster_scores(X, seq)), arrays(mt.cluster_scores(X, mt.label2str(seq))), 'sequence labels')


# ------------------------------------------------------------------------------------------------ pt_corr
def with_correlation(target, rhos, rng):
    """A dataset of target's shape whose condition c has Pearson r = rhos[c] with target's (up to rounding): the centred,
    normalised condition mixed with a unit vector orthogonal to it and to the constant, then scaled and shifted."""
    out = np.empty(target.shape)
    for c, rho in enumerate(rhos):
        x = target[c].ravel()
        u = (x - x.mean()) / np.linalg.norm(x - x.mean())
        w = rng.standard_normal(x.size)
        w = w - w.mean()
        w = w - (w @ u) * u
        out[c] = (3.0 + 2.0 * (rho * u + np.sqrt(1.0 - rho * rho) * w / np.linalg.norm(w))).reshape(target.shape[1:])
    return out


@pytest.mark.parametrize('d', (1, 6))
def test_pt_corr_follows_scipy(d):
    """r within 4 (T d + 4) u of scipy per condition, and the p-value within the same RELATIVE bar.  p = 2 sf(|r|) answers a
    change of r with the factor |d ln p / d r| = 2 pdf(r) / p, which grows without bound towards |r| = 1 (7 at |r| = 0.8 for
    T d = 5, 40 at |r| = 0.6 for T d = 30), while two float64 evaluations of r differ by a few u whatever the recipe.  A relative
    bar on p equal to the bar on r can therefore only be asked where that factor is a small multiple of one: the two datasets
    whose p-values are held to it have correlations built to lie in [-0.3, 0.3].  The third is strongly correlated, as
    aligned data are; its r is held to the same bar and its p-values to the formula itself, evaluated at the function's own r."""
    from scipy import special
    mt = MT()
    n_c, T = 7, 5
    rng = np.random.default_rng(40 + d)
    target = rng.standard_normal((n_c, T, d))
    rhos = np.linspace(-0.3, 0.3, n_c)
    others = [with_correlation(target, rhos, rng), with_correlation(target, -rhos[::-1] * 0.5, rng).astype(np.float32),
              0.9 * target + 0.3 * rng.standard_normal((n_c, T, d))]
    bar = 4 * (T * d + 4) * U
    plain = mt.pt_corr(target, others[0])
    assert isinstance(plain, np.ndarray) and plain.shape == (n_c,) and plain.dtype == np.float64
    rs, ps = mt.pt_corr_multi(target, others, p_vals=True)
    assert isinstance(rs, list) and isinstance(ps, list) and len(rs) == len(ps) == 3
    only_r = mt.pt_corr_multi(target, others)
    assert isinstance(only_r, list) and len(only_r) == 3
    worst_r = worst_p = 0.0
    for i, o in enumerate(others):
        r1, p1 = mt.pt_corr(target, o, p_vals=True)
        assert r1.shape == p1.shape == (n_c,) and r1.dtype == p1.dtype == np.float64
        assert np.array_equal(bits(r1), bits(rs[i])) and np.array_equal(bits(p1), bits(ps[i]))       # list form = single form
        assert np.array_equal(bits(only_r[i]), bits(rs[i])) and np.array_equal(bits(mt.pt_corr(target, o)), bits(r1))
        ab = T * d / 2 - 1
        assert np.array_equal(bits(p1), bits(2 * special.betaincc(ab, ab, (np.abs(r1) + 1) / 2)))    # scipy's beta distribution
        for c in range(n_c):
            ref = stats.pearsonr(target[c].flatten(), o[c].astype(np.float64).flatten())
            worst_r = max(worst_r, abs(r1[c] - ref.statistic) / bar)
            assert abs(r1[c] - ref.statistic) <= bar
            if i < 2 and ref.pvalue > 1e-300:
                worst_p = max(worst_p, abs(p1[c] - ref.pvalue) / ref.pvalue / bar)
                assert abs(p1[c] - ref.pvalue) <= bar * ref.pvalue
    assert (np.abs(rs[2]) > 0.7).all() and (np.abs(rs[0] - rhos) < 1e-12).all()
    print(f'd={d}: largest fraction of the bar: r {worst_r:.3f}, p {worst_p:.3f}')
