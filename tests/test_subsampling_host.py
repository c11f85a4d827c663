"""processing_utils on the host: the index generators and both *_sig_channels functions against the reference's own output
(tests/golden/subsampling.npz, made by tests/golden/make_subsampling_fixtures.py), the plain-numpy restatement of the
mean the kernels follow against the spatial_avg_data goldens BIT FOR BIT, and the argument checks.  No GPU needed."""
import os

import numpy as np
import pytest
import torch

from cross_patient_speech_decoding_amd import processing_utils as PU
from cross_patient_speech_decoding_amd.processing_utils import grid_subsampling as GS
from cross_patient_speech_decoding_amd.processing_utils import spatial_avg_subsampling as SA

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden', 'subsampling.npz')
PATIENTS = ('P1', 'P2', 'P3')
MEAN_GROUPINGS = ('c1', 'c2', 'c3', 'c8', 'r2', 'r3')


def load_golden():
    return np.load(GOLDEN)


def load_list(z, name):
    """The list of index arrays stored as <name>_cat / <name>_len."""
    return np.split(z[name + '_cat'], np.cumsum(z[name + '_len'])[:-1]) if len(z[name + '_len']) else []


def mean_grouping(z, name):
    """Index arrays of a mean<..>_<name> golden: full groups c<k> of the (8, 16) grid, ragged NaN-dropped groups r<k>."""
    return load_list(z, f'avg_8x16_{name}' if name[0] == 'c' else f'asig_P3_c{name[1]}')


def restate_mean(data, avgIdxs):
    """spatial_avg_data restated: the members of a group added ONE BY ONE IN MEMBER ORDER in the input's dtype (what numpy's
    add.reduce does along an axis that is not the contiguous one: no pairwise summation), one division by the member count
    in that dtype, then widened to float64 by the assignment into the float64 result; (trials, time, groups)."""
    data = np.asarray(data)
    out = np.empty((data.shape[0], data.shape[3], len(avgIdxs)), dtype=np.float64)
    for g, idxs in enumerate(avgIdxs):
        acc = data[:, idxs[0, 0], idxs[0, 1], :].copy()
        for ix, iy in idxs[1:]:
            acc = acc + data[:, ix, iy, :]
        assert acc.dtype == data.dtype
        out[:, :, g] = acc / data.dtype.type(len(idxs))
    return out


def assert_same_lists(got, want):
    assert len(got) == len(want)
    for a, b in zip(got, want):
        a = np.asarray(a)
        assert a.shape == b.shape and np.issubdtype(a.dtype, np.integer)
        assert np.array_equal(a, b)


@pytest.fixture(scope='module')
def z():
    return load_golden()


def test_grid_susbsample_idxs_matches_reference(z):
    assert_same_lists(PU.grid_susbsample_idxs((8, 16), (6, 12), step=(1, 1)), load_list(z, 'grid_a'))
    assert_same_lists(PU.grid_susbsample_idxs((8, 16), (6, 12)), load_list(z, 'grid_a'))
    assert_same_lists(PU.grid_susbsample_idxs((12, 22), (4, 8), step=(2, 3), start=(1, 2)), load_list(z, 'grid_b'))
    assert_same_lists(PU.grid_susbsample_idxs((8, 16), (8, 16)), load_list(z, 'grid_c'))
    assert len(load_list(z, 'grid_a')) == 15 and len(load_list(z, 'grid_c')) == 1


@pytest.mark.parametrize('grid', [(8, 16), (12, 22)])
@pytest.mark.parametrize('k', [1, 2, 3, 8])
def test_spatial_avg_idxs_matches_reference(z, grid, k):
    assert_same_lists(PU.spatial_avg_idxs(grid, k), load_list(z, f'avg_{grid[0]}x{grid[1]}_c{k}'))


def _write_mats(tmp_path, z, pt):
    import scipy.io as sio
    os.makedirs(tmp_path / pt)
    sio.savemat(str(tmp_path / pt / f'{pt}_channelMap.mat'), {'chanMap': z[f'map_{pt}']})
    sio.savemat(str(tmp_path / pt / f'{pt}_sigChannel.mat'), {'sigChannel': z[f'sig_{pt}']})


@pytest.mark.parametrize('form', ['arrays', 'mat'])
@pytest.mark.parametrize('pt', PATIENTS)
def test_grid_subsample_sig_channels_matches_reference(z, tmp_path, pt, form):
    if form == 'mat':
        _write_mats(tmp_path, z, pt)
        kw, path = {}, str(tmp_path)
    else:
        kw, path = dict(chanMap=z[f'map_{pt}'], sigChannel=z[f'sig_{pt}']), '/nonexistent'
    assert_same_lists(PU.grid_subsample_sig_channels(pt, (4, 6), path, **kw), load_list(z, f'gsig_{pt}'))
    assert_same_lists(PU.grid_subsample_sig_channels(pt, (4, 6), path, step=(2, 3), **kw), load_list(z, f'gsig_{pt}_step'))


@pytest.mark.parametrize('form', ['arrays', 'mat'])
@pytest.mark.parametrize('pt', PATIENTS)
def test_spatial_avg_sig_channels_matches_reference(z, tmp_path, pt, form):
    if form == 'mat':
        _write_mats(tmp_path, z, pt)
        kw, path = {}, str(tmp_path)
    else:
        kw, path = dict(chanMap=z[f'map_{pt}'], sigChannel=z[f'sig_{pt}']), '/nonexistent'
    for k in (2, 3):
        assert_same_lists(PU.spatial_avg_sig_channels(pt, k, path, useSig=True, **kw), load_list(z, f'asig_{pt}_c{k}'))
    # useSig=False reads no significant-channel file at all
    kw.pop('sigChannel', None)
    assert_same_lists(PU.spatial_avg_sig_channels(pt, 3, path, **kw), load_list(z, f'asig_{pt}_c3_all'))


def test_goldens_hold_ragged_groups(z):
    sizes = z['asig_P3_c3_len'].tolist()
    assert 5 in sizes and 9 in sizes           # a 3 x 3 region with four NaN cells keeps five members


@pytest.mark.parametrize('tag', ['64', '32'])
@pytest.mark.parametrize('name', MEAN_GROUPINGS)
def test_restatement_equals_reference_mean_bitwise(z, name, tag):
    data, want = z['data' + tag], z[f'mean{tag}_{name}']
    assert data.dtype == (np.float64 if tag == '64' else np.float32) and want.dtype == np.float64
    got = restate_mean(data, mean_grouping(z, name))
    assert got.shape == want.shape
    assert np.array_equal(got.view(np.int64), want.view(np.int64))


def test_float32_mean_is_accumulated_in_float32(z):
    """The float32 golden is NOT the float64 mean of the float32 values: the kernel must accumulate in the input's dtype."""
    wide = restate_mean(z['data32'].astype(np.float64), mean_grouping(z, 'c3'))
    assert not np.array_equal(wide, z['mean32_c3'])


def _data(shape=(2, 4, 6, 5)):
    return np.arange(np.prod(shape), dtype=np.float64).reshape(shape)


@pytest.mark.parametrize('make', [np.asarray, torch.from_numpy], ids=['numpy', 'torch'])
def test_spatial_avg_argument_checks_raise_value_error(make):
    d = make(_data())
    good = PU.spatial_avg_idxs((4, 6), 2)
    for fn, wrap in ((SA.spatial_avg_data, lambda g: g), (SA.spatial_avg_sweep, lambda g: [good, g])):
        with pytest.raises(ValueError, match='outside'):
            fn(d, wrap([np.array([[0, 0], [4, 0]])]))                 # row 4 of a 4-row grid
        with pytest.raises(ValueError, match='outside'):
            fn(d, wrap([np.array([[0, 6]])]))
        with pytest.raises(ValueError, match='outside'):
            fn(d, wrap([np.array([[-1, 0]])]))
        with pytest.raises(ValueError, match='empty'):
            fn(d, wrap(good + [np.zeros((0, 2), dtype=np.int64)]))
        with pytest.raises(ValueError, match='no groups'):
            fn(d, wrap([]))
        with pytest.raises(ValueError, match='dimensions'):
            fn(make(_data()[0]), wrap(good))
    with pytest.raises(ValueError, match='no groupings'):
        SA.spatial_avg_sweep(d, [])


@pytest.mark.parametrize('make', [np.asarray, torch.from_numpy], ids=['numpy', 'torch'])
def test_select_channels_argument_checks_raise_value_error(make):
    X = make(np.zeros((3, 5, 7), dtype=np.float32))
    with pytest.raises(ValueError, match='no index arrays'):
        GS.select_channels_sweep(X, [])
    with pytest.raises(ValueError, match='empty'):
        GS.select_channels_sweep(X, [np.array([0, 1]), np.array([], dtype=np.int64)])
    with pytest.raises(ValueError, match='outside'):
        GS.select_channels_sweep(X, [np.array([0, 7])])
    with pytest.raises(ValueError, match='outside'):
        GS.select_channels_sweep(X, [np.array([-1])])
    with pytest.raises(ValueError, match='dimensions'):
        GS.select_channels_sweep(make(np.zeros((3, 5), dtype=np.float32)), [np.array([0])])


def test_no_cpu_fallback():
    """Valid arguments reach the device: without one the package's usual RuntimeError, never a host computation."""
    d, groups = _data(), PU.spatial_avg_idxs((4, 6), 2)
    if torch.cuda.is_available():
        assert np.array_equal(PU.spatial_avg_data(d, groups), restate_mean(d, groups))
    else:
        with pytest.raises(RuntimeError, match='no CPU fallback'):
            PU.spatial_avg_data(d, groups)
        with pytest.raises(RuntimeError, match='no CPU fallback'):
            PU.spatial_avg_sweep(d, [groups])
        with pytest.raises(RuntimeError, match='no CPU fallback'):
            PU.select_channels_sweep(np.zeros((3, 5, 7), dtype=np.float32), [np.array([0, 1])])
