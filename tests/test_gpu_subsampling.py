"""Electrode subsampling on the MI355X (csrc/xps_subsample.hip through processing_utils): spatial_avg_data against the
reference's own output and against the plain-numpy restatement of its arithmetic (tests/test_subsampling_host.py proves the
two equal), the sweeps against the single calls and against X[:, :, idx].  Every comparison is exact equality of bits."""
import numpy as np
import pytest
import torch
from sklearn.ensemble import BaggingClassifier

from test_subsampling_host import MEAN_GROUPINGS, load_golden, load_list, mean_grouping, restate_mean

pytestmark = pytest.mark.gpu


@pytest.fixture(scope='module')
def z():
    return load_golden()


@pytest.fixture(scope='module')
def PU():
    from cross_patient_speech_decoding_amd import processing_utils
    return processing_utils


def bits_equal(got, want):
    """torch.equal on the bit patterns (so that a NaN or a signed zero cannot hide a difference)."""
    want = torch.from_numpy(np.array(want, order='C', copy=True))             # (a fresh copy: canonical strides)
    got = got.cpu() if isinstance(got, torch.Tensor) else torch.from_numpy(np.array(got, order='C', copy=True))
    if got.dtype != want.dtype or got.shape != want.shape:
        return False
    as_int = torch.int64 if want.dtype == torch.float64 else torch.int32
    return torch.equal(got.contiguous().view(as_int), want.view(as_int))


@pytest.mark.parametrize('where', ['numpy', 'device'])
@pytest.mark.parametrize('tag', ['64', '32'])
@pytest.mark.parametrize('name', MEAN_GROUPINGS)
def test_spatial_avg_data_equals_reference_bitwise(z, PU, name, tag, where):
    data, want = z['data' + tag], z[f'mean{tag}_{name}']
    groups = mean_grouping(z, name)
    if where == 'numpy':
        got = PU.spatial_avg_data(data, groups)
        assert isinstance(got, np.ndarray) and got.dtype == np.float64
    else:
        got = PU.spatial_avg_data(torch.from_numpy(data).cuda(), groups)
        assert isinstance(got, torch.Tensor) and got.is_cuda and got.dtype == torch.float64 and got.is_contiguous()
    assert bits_equal(got, want)


@pytest.mark.parametrize('tag', ['64', '32'])
def test_sweep_equals_single_calls_bitwise(z, PU, tag):
    data = torch.from_numpy(z['data' + tag]).cuda()
    groupings = [mean_grouping(z, name) for name in MEAN_GROUPINGS]
    slabs = PU.spatial_avg_sweep(data, groupings)
    assert len(slabs) == len(groupings)
    base = slabs[0].data_ptr()
    for name, groups, slab in zip(MEAN_GROUPINGS, groupings, slabs):
        assert slab.is_cuda and slab.dtype == torch.float64 and slab.is_contiguous()
        assert tuple(slab.shape) == (6, 25, len(groups))                         # channel-last
        assert slab.data_ptr() == base                                           # views of ONE slab, back to back
        base += slab.numel() * 8
        assert bits_equal(slab, PU.spatial_avg_data(data, groups).cpu().numpy())
        assert bits_equal(slab, z[f'mean{tag}_{name}'])
    host = PU.spatial_avg_sweep(z['data' + tag], groupings)                      # host input: uploaded once, device tensors out
    assert all(h.is_cuda and bits_equal(h, s.cpu().numpy()) for h, s in zip(host, slabs))


@pytest.mark.parametrize('dtype', [np.float32, np.float64])
def test_select_channels_sweep_equals_indexing(z, PU, dtype):
    rng = np.random.default_rng(5)
    X = rng.standard_normal((7, 37, 128)).astype(dtype)
    windows = [idx[:, 0] * 16 + idx[:, 1] for idx in load_list(z, 'grid_a')]     # every (6, 12) window of the (8, 16) grid
    assert len(windows) == 15
    outs = PU.select_channels_sweep(torch.from_numpy(X).cuda(), windows)
    assert len(outs) == len(windows)
    for idx, out in zip(windows, outs):
        assert out.is_cuda and out.is_contiguous() and tuple(out.shape) == (7, 37, 72)
        assert bits_equal(out, X[:, :, idx])
    outs = PU.select_channels_sweep(X, [np.array([5]), np.arange(128)[::-1], np.array([3, 3, 127, 0])])
    assert bits_equal(outs[0], X[:, :, [5]]) and bits_equal(outs[1], X[:, :, ::-1]) and bits_equal(outs[2], X[:, :, [3, 3, 127, 0]])


def _groups_of_flat(Y, flat_groups):
    return [np.stack([np.asarray(g) // Y, np.asarray(g) % Y], axis=1) for g in flat_groups]


AWKWARD = {
    # name: (N, X, Y, T, groups as flat channel numbers)
    'T1': (5, 4, 6, 1, [[0, 1, 6, 7], [2, 3, 8, 9, 23], list(range(24))]),
    'T_not_tile_multiple': (3, 4, 6, 45, [[0, 1, 6, 7], [22, 23], [5]]),
    'T_one_past_tile': (3, 4, 6, 33, [[0, 1, 6, 7], [22, 23], [5]]),
    'C1': (4, 1, 1, 19, [[0], [0]]),
    'G1': (4, 4, 6, 19, [[3, 9, 15]]),
    'all_channels_in_one_group': (4, 5, 7, 19, [list(range(35))[::-1]]),
    'channel_in_several_groups': (4, 4, 6, 19, [[0, 1, 2], [2, 1, 0], [1], [1, 1, 1], [1, 23]]),
    'C_not_divisible_by_4': (4, 3, 7, 40, [[0, 20], [1, 2, 3, 4, 5], [19, 18, 17], [6]]),
    'many_channels_small_tile': (2, 30, 30, 21, [list(range(0, 900, 7)), [899, 0], list(range(450, 500))]),
}


@pytest.mark.parametrize('dtype', [np.float32, np.float64])
@pytest.mark.parametrize('case', sorted(AWKWARD))
def test_awkward_shapes_equal_restatement_bitwise(PU, case, dtype):
    N, X, Y, T, flat = AWKWARD[case]
    rng = np.random.default_rng(len(case))
    data = (rng.standard_normal((N, X, Y, T)) * 2.0 - 0.25).astype(dtype)
    groups = _groups_of_flat(Y, flat)
    want = restate_mean(data, groups)
    assert bits_equal(PU.spatial_avg_data(data, groups), want)
    sweep = PU.spatial_avg_sweep(data, [groups, groups[::-1]])
    assert bits_equal(sweep[0], want) and bits_equal(sweep[1], want[:, :, ::-1])


@pytest.mark.parametrize('dtype', [np.float32, np.float64])
def test_non_contiguous_input_is_not_misread(PU, dtype):
    rng = np.random.default_rng(9)
    base = rng.standard_normal((4, 21, 5, 6)).astype(dtype)                      # (N, T, X, Y) in memory
    data = base.transpose(0, 2, 3, 1)                                            # (N, X, Y, T) view, T not contiguous
    groups = PU.spatial_avg_idxs((5, 6), 2)
    want = restate_mean(np.ascontiguousarray(data), groups)
    assert bits_equal(PU.spatial_avg_data(data, groups), want)
    dev = torch.from_numpy(base).cuda().permute(0, 2, 3, 1)
    assert not dev.is_contiguous()
    assert bits_equal(PU.spatial_avg_data(dev, groups), want)
    assert bits_equal(PU.spatial_avg_sweep(dev[:, ::2], [PU.spatial_avg_idxs((3, 6), 3)])[0],
                      restate_mean(np.ascontiguousarray(data[:, ::2]), PU.spatial_avg_idxs((3, 6), 3)))
    Xf = rng.standard_normal((4, 9, 30)).astype(dtype)
    got = PU.select_channels_sweep(torch.from_numpy(Xf).cuda()[:, :, ::3], [np.array([0, 9, 4])])[0]
    assert bits_equal(got, Xf[:, :, ::3][:, :, [0, 9, 4]])


@pytest.mark.parametrize('dtype', [np.float32, np.float64])
def test_realistic_sweep_equals_restatement_bitwise(PU, dtype):
    rng = np.random.default_rng(12)
    data = rng.standard_normal((512, 12, 24, 200)).astype(dtype)
    groupings = [PU.spatial_avg_idxs((12, 24), k) for k in range(1, 7)]
    slabs = PU.spatial_avg_sweep(torch.from_numpy(data).cuda(), groupings)
    for k, (groups, slab) in enumerate(zip(groupings, slabs), 1):
        assert tuple(slab.shape) == (512, 200, (12 // k) * (24 // k))
        assert bits_equal(slab, restate_mean(data, groups)), f'contact size {k}'


def test_deterministic_and_stream_independent(z, PU):
    data = torch.from_numpy(z['data32']).cuda()
    groupings = [mean_grouping(z, name) for name in MEAN_GROUPINGS]
    X = torch.randn(6, 25, 128, device='cuda')
    windows = [idx[:, 0] * 16 + idx[:, 1] for idx in load_list(z, 'grid_a')]
    first = [t.clone() for t in PU.spatial_avg_sweep(data, groupings) + PU.select_channels_sweep(X, windows)]
    single = PU.spatial_avg_data(data, groupings[2]).clone()
    again = PU.spatial_avg_sweep(data, groupings) + PU.select_channels_sweep(X, windows)
    assert all(bits_equal(a, b.cpu().numpy()) for a, b in zip(again, first))
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        other = PU.spatial_avg_sweep(data, groupings) + PU.select_channels_sweep(X, windows)
        other_single = PU.spatial_avg_data(data, groupings[2])
    side.synchronize()
    assert all(bits_equal(a, b.cpu().numpy()) for a, b in zip(other, first))
    assert bits_equal(other_single, single.cpu().numpy())


def test_sweep_feeds_cross_patient_decoder_like_the_host_path(PU):
    """One contact size of a sweep through the device path and the same grouping averaged with numpy on the host: the
    aligned cross-patient SVM decode (crossPtDecoder_sepAlign around the device SVC) predicts the same labels."""
    import cross_patient_speech_decoding_amd.alignment as A
    from cross_patient_speech_decoding_amd.decoders import SVC as DeviceSVC
    from cross_patient_speech_decoding_amd.decoders import crossPtDecoder_sepAlign
    from cross_patient_speech_decoding_amd.utils.synthetic import make_patient
    grid, T = (4, 8), 14
    pats = []
    for p in range(3):
        x, y = make_patient(p, 72 - 6 * p, T=T, C=grid[0] * grid[1], n_cond=9, noise=2.0)
        pats.append((np.ascontiguousarray(x.astype(np.float64).transpose(0, 2, 1)).reshape(len(x), *grid, T), y))
    groupings = [PU.spatial_avg_idxs(grid, k) for k in (1, 2, 4)]
    dev = [PU.spatial_avg_sweep(raw, groupings)[1].cpu().numpy() for raw, _ in pats]
    host = [restate_mean(raw, groupings[1]) for raw, _ in pats]
    assert all(d.shape == (len(raw), T, 8) for d, (raw, _) in zip(dev, pats))

    def predictions(feats):
        (Xt, yt), cross = (feats[0], pats[0][1]), [(f, y[:, 0], y) for f, (_, y) in zip(feats[1:], pats[1:])]
        clf = BaggingClassifier(DeviceSVC(kernel='linear'), n_estimators=10, random_state=0)
        dec = crossPtDecoder_sepAlign(cross, clf, A.AlignCCA, n_comp=0.9)
        tr, te = np.arange(0, 54), np.arange(54, 72)
        dec.fit(Xt[tr], yt[tr, 0], y_align=yt[tr])
        return dec.predict(Xt[te])
    p_dev, p_host = predictions(dev), predictions(host)
    assert p_dev.shape == (18,)
    np.testing.assert_array_equal(p_dev, p_host)
