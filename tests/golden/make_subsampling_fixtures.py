"""Generate tests/golden/subsampling.npz from the REFERENCE's processing_utils/grid_subsampling.py and
spatial_avg_subsampling.py.
Build container only:  python tests/golden/make_subsampling_fixtures.py <reference checkout>/aligned_decoding
(or REFERENCE_ALIGNED_DECODING in the environment).

Both modules import matplotlib.pyplot for their __main__ demos only; where matplotlib is absent an empty in-process glue
module stands in.  The glue touches no arithmetic: every stored array is what the reference's own code computed with numpy /
scipy on the CPU.

A list of index arrays is stored as <name>_cat (the arrays concatenated along axis 0) and <name>_len (their lengths).
Contents:
  grid_a / grid_b / grid_c     grid_susbsample_idxs: (8,16) / (6,12) / step 1; (12,22) / (4,8) / step (2,3) / start (1,2);
                               window = grid (8,16)
  avg_<X>x<Y>_c<k>             spatial_avg_idxs for contact sizes 1, 2, 3, 8 on (8,16) and (12,22)
  map_<pt>, sig_<pt>           channel maps (NaN = no electrode) and significant-channel lists of three synthetic patients,
                               written to temporary .mat files for the reference: P1 24 x 10 (first side 24 wide: rows
                               trimmed, window transposed), P2 12 x 24 (second side 24 wide), P3 8 x 16; NaN corners in all
  gsig_<pt>                    grid_subsample_sig_channels(pt, (4, 6), path[, step])
  asig_<pt>_c<k>[_all]         spatial_avg_sig_channels(pt, k, path, useSig=True) ([_all]: useSig=False)
  data64 / data32              (6, 8, 16, 25) raw trials, float64 and its float32 rounding
  mean64_<g> / mean32_<g>      spatial_avg_data(data, groups) for g in c1, c2, c3, c8 (full groups of avg_8x16_c<k>) and
                               r2, r3 (ragged NaN-dropped groups asig_P3_c2 / asig_P3_c3)"""
import os
import sys
import tempfile
import types

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))


def _glue():
    try:
        import matplotlib.pyplot  # noqa: F401
    except ImportError:
        mpl, plt = types.ModuleType('matplotlib'), types.ModuleType('matplotlib.pyplot')
        mpl.pyplot = plt
        sys.modules.update({'matplotlib': mpl, 'matplotlib.pyplot': plt})


def _put(out, name, arrays):
    arrays = [np.asarray(a) for a in arrays]
    out[name + '_len'] = np.array([len(a) for a in arrays], dtype=np.int64)
    out[name + '_cat'] = np.concatenate(arrays, axis=0) if arrays else np.zeros((0, 2), dtype=np.int64)


def _chan_map(rng, shape, trim_axis, corner):
    """Channel numbers 1..n in random order over the electrode cells; NaN on the trimmed border and in the corner blocks."""
    m = np.ones(shape, dtype=bool)
    if trim_axis == 0:
        m[0, :] = m[-1, :] = False
    elif trim_axis == 1:
        m[:, 0] = m[:, -1] = False
    inner = m[1:-1, :] if trim_axis == 0 else m[:, 1:-1] if trim_axis == 1 else m
    (a, b), (c, d) = corner
    inner[:a, :b] = False
    inner[-c:, -d:] = False
    cm = np.full(shape, np.nan)
    cm[m] = rng.permutation(int(m.sum())) + 1
    return cm


if __name__ == '__main__':
    ref = sys.argv[1] if len(sys.argv) > 1 else os.environ.get('REFERENCE_ALIGNED_DECODING')
    if not ref or not os.path.isdir(os.path.join(ref, 'processing_utils')):
        sys.exit('usage: make_subsampling_fixtures.py <reference checkout>/aligned_decoding')
    _glue()
    sys.path.insert(0, ref)
    import scipy
    import scipy.io as sio
    from processing_utils import grid_subsampling as RG                 # noqa: E402
    from processing_utils import spatial_avg_subsampling as RS          # noqa: E402

    out = dict(numpy_version=np.array(np.__version__), scipy_version=np.array(scipy.__version__))
    rng = np.random.default_rng(2026)

    _put(out, 'grid_a', RG.grid_susbsample_idxs((8, 16), (6, 12), step=(1, 1)))
    _put(out, 'grid_b', RG.grid_susbsample_idxs((12, 22), (4, 8), step=(2, 3), start=(1, 2)))
    _put(out, 'grid_c', RG.grid_susbsample_idxs((8, 16), (8, 16)))
    for grid in ((8, 16), (12, 22)):
        for k in (1, 2, 3, 8):
            _put(out, f'avg_{grid[0]}x{grid[1]}_c{k}', RS.spatial_avg_idxs(grid, k))

    tmp = tempfile.mkdtemp()
    pts = {'P1': ((24, 10), 0, ((3, 2), (2, 2))), 'P2': ((12, 24), 1, ((2, 3), (1, 2))), 'P3': ((8, 16), None, ((3, 2), (2, 3)))}
    for pt, (shape, trim, corner) in pts.items():
        cm = _chan_map(rng, shape, trim, corner)
        n = int(np.nanmax(cm))
        sig = np.sort(rng.choice(np.arange(1, n + 1), size=16, replace=False)).astype(np.float64)[None, :]
        os.makedirs(os.path.join(tmp, pt))
        sio.savemat(os.path.join(tmp, pt, f'{pt}_channelMap.mat'), {'chanMap': cm})
        sio.savemat(os.path.join(tmp, pt, f'{pt}_sigChannel.mat'), {'sigChannel': sig})
        out[f'map_{pt}'], out[f'sig_{pt}'] = cm, sig
        _put(out, f'gsig_{pt}', RG.grid_subsample_sig_channels(pt, (4, 6), tmp))
        _put(out, f'gsig_{pt}_step', RG.grid_subsample_sig_channels(pt, (4, 6), tmp, step=(2, 3)))
        for k in (2, 3):
            _put(out, f'asig_{pt}_c{k}', RS.spatial_avg_sig_channels(pt, k, tmp, useSig=True))
        _put(out, f'asig_{pt}_c3_all', RS.spatial_avg_sig_channels(pt, 3, tmp))

    data = rng.standard_normal((6, 8, 16, 25)) * 3.0 + 0.5
    out['data64'], out['data32'] = data, data.astype(np.float32)
    groupings = {f'c{k}': RS.spatial_avg_idxs((8, 16), k) for k in (1, 2, 3, 8)}
    groupings.update(r2=RS.spatial_avg_sig_channels('P3', 2, tmp, useSig=True),
                     r3=RS.spatial_avg_sig_channels('P3', 3, tmp, useSig=True))
    assert len({len(g) for g in groupings['r3']}) > 1, 'the ragged grouping is not ragged'
    for name, groups in groupings.items():
        for tag in ('64', '32'):
            res = RS.spatial_avg_data(out['data' + tag], groups)
            assert res.dtype == np.float64 and res.shape == (6, 25, len(groups))
            out[f'mean{tag}_{name}'] = res

    path = os.path.join(HERE, 'subsampling.npz')
    np.savez_compressed(path, **out)
    print('subsampling.npz', os.path.getsize(path), 'bytes;', len(out), 'arrays; ragged sizes',
          [len(g) for g in groupings['r3']])
