"""decoders._ovo, the host side (no GPU): the one class-pair problem builder of SVC, BaggingClassifier and SVCSearchCV against a
brute-force restatement of its rules (a loop over the kept rows), and the bound C * class weight * sample weight bit for bit."""
import numpy as np
import pytest

from cross_patient_speech_decoding_amd.decoders import _ovo

LABELS, SIZES, C = (1, 4, 7), (30, 28, 2), 0.7


def data():
    """Class indices of 60 shuffled rows, classes 1 / 4 / 7 of 30 / 28 / 2 rows."""
    yi = np.repeat(np.arange(3), SIZES)
    return yi[np.random.default_rng(3).permutation(len(yi))]


def weights_of(class_weight, yi):
    """sklearn's compute_class_weight for the three settings, restated."""
    if class_weight is None:
        return np.ones(3)
    if class_weight == 'balanced':
        return np.array([len(yi) / (3 * float((yi == c).sum())) for c in range(3)])
    return np.array([float(class_weight.get(label, 1.0)) for label in LABELS])


def brute_force(yi, positions, cw, w):
    """The rules, row by row: zero-weight rows dropped; classes ascending, the lower class of a pair first (positive); rows in
    original order inside a class; a class without rows has no pairs; the bound is C * cw[class] * w."""
    kept = [r for r in range(len(yi)) if w[r] > 0]
    present = sorted({int(yi[r]) for r in kept})
    idx, cb, sizes, npos, pairs = [], [], [], [], []
    for i, a in enumerate(present):
        for b in present[i + 1:]:
            first, second = [r for r in kept if yi[r] == a], [r for r in kept if yi[r] == b]
            idx += [int(positions[r]) for r in first + second]
            cb += [C * float(cw[yi[r]]) * float(w[r]) for r in first + second]
            sizes.append(len(first) + len(second))
            npos.append(len(first))
            pairs.append((a, b))
    return idx, cb, sizes, npos, pairs


def sample_weights(kind, yi):
    if kind == 'none':
        return None
    w = np.random.default_rng(11).integers(0, 4, len(yi)).astype(np.float64)      # integers 0..3: some rows dropped, some counted thrice
    assert (w == 0).any() and (w > 1).any()
    w[yi == {'lose-last': 2, 'lose-first': 0}[kind]] = 0.0                          # the class loses all its weight
    return w


@pytest.mark.parametrize('order', ['identity', 'descending'])
@pytest.mark.parametrize('kind', ['none', 'lose-last', 'lose-first'])
@pytest.mark.parametrize('class_weight', [None, 'balanced', {4: 2.5}], ids=['none', 'balanced', 'dict'])
def test_builder_equals_the_rules_row_by_row(class_weight, kind, order):
    yi = data()
    n = len(yi)
    positions = np.arange(n) if order == 'identity' else np.arange(n)[::-1].copy()
    cw = weights_of(class_weight, yi)
    np.testing.assert_array_equal(_ovo.class_weights(class_weight, np.array(LABELS), yi), cw)
    w = sample_weights(kind, yi)
    idx, cb, sizes, npos, pairs = brute_force(yi, positions, cw, np.ones(n) if w is None else w)
    p = _ovo.pair_problems(yi, positions, cw, w)
    assert pairs == {'none': [(0, 1), (0, 2), (1, 2)], 'lose-last': [(0, 1)], 'lose-first': [(1, 2)]}[kind]   # indices into the FULL class list
    assert p['idx'].dtype == np.int32
    np.testing.assert_array_equal(p['idx'], idx)
    np.testing.assert_array_equal(p['sizes'], sizes)
    np.testing.assert_array_equal(p['npos'], npos)
    assert list(zip(p['pair_a'].tolist(), p['pair_b'].tolist())) == pairs
    got = _ovo.bounds(C, p)
    assert got.dtype == np.float64 and (got > 0).all()
    np.testing.assert_array_equal(got.view(np.int64), np.array(cb).view(np.int64))           # bit for bit
    if kind == 'none':
        assert sorted(p['sizes'].tolist()) == [30, 32, 58] and len(idx) == 2 * n


def test_fewer_than_two_classes_raise_sklearns_error():
    yi = data()
    n = len(yi)
    with pytest.raises(ValueError, match='The number of classes has to be greater than one; got 1 class'):
        _ovo.pair_problems(yi, np.arange(n), np.ones(3), (yi == 1).astype(np.float64))
    with pytest.raises(ValueError, match='The number of classes has to be greater than one; got 1 class'):
        _ovo.pair_problems(np.zeros(5, dtype=np.int64), np.arange(5), np.ones(1))
    with pytest.raises(ValueError, match='The number of classes has to be greater than one; got 0 class'):
        _ovo.pair_problems(yi, np.arange(n), np.ones(3), np.zeros(n))
