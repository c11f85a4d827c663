"""Spatial averaging of electrode channels over square contact regions (reference
processing_utils/spatial_avg_subsampling.py).

The index lists are built on the host; spatial_avg_data runs on the MI355X (xps_group_mean_*: one pass over the raw
(trials, X, Y, T) tensor, channel-last float64 out, the reference's bits), and spatial_avg_sweep serves every contact size of
a sweep from one launch that reads the resident tensor once.  There is no CPU fallback."""
import numpy as np
import torch

from .._lib import call
from .grid_subsampling import _sig_channels, _trimmed_chan_map, grid_susbsample_idxs


def spatial_avg_idxs(gridSize, contactSize):
    """(row, col) index arrays of the non-overlapping contactSize x contactSize regions of a grid, the tiling centred in it."""
    shift = ((gridSize[0] % contactSize) // 2, (gridSize[1] % contactSize) // 2)
    return grid_susbsample_idxs(gridSize, (contactSize, contactSize), (contactSize, contactSize), shift)


def spatial_avg_sig_channels(pt, contactSize, dataPath, useSig=False, *, chanMap=None, sigChannel=None):
    """Grid index arrays of the patient's averaging regions.  useSig: regions with at least half their cells NaN are skipped,
    NaN cells are dropped from the others (ragged groups), and only regions holding a significant channel are kept.
    ``chanMap`` / ``sigChannel`` arrays replace the .mat files under {dataPath}/{pt}/."""
    chanMap, _ = _trimmed_chan_map(pt, dataPath, chanMap)
    regions = spatial_avg_idxs(chanMap.shape, contactSize)
    if not useSig:
        return regions
    sig = _sig_channels(pt, dataPath, sigChannel)
    kept = []
    for idxs in regions:
        elec = chanMap[idxs[:, 0], idxs[:, 1]]
        bad = np.isnan(elec)
        if bad.sum() >= len(elec) / 2:
            continue
        if np.intersect1d(sig, elec[~bad].astype(int)).size > 0:
            kept.append(idxs[~bad])
    return kept


def _csr(shape, avgIdxs, who):
    """(offsets, members) of one grouping: flat row-major channel numbers of every group.  Raises ValueError."""
    X, Y = int(shape[1]), int(shape[2])
    offsets, members = [0], []
    for g, idxs in enumerate(avgIdxs):
        idxs = np.asarray(idxs)
        if idxs.size == 0:
            raise ValueError(f'{who}: group {g} is empty')
        if idxs.ndim != 2 or idxs.shape[1] != 2 or not np.issubdtype(idxs.dtype, np.integer):
            raise ValueError(f'{who}: group {g} must be an integer (members, 2) array of grid indices')
        if idxs.min() < 0 or idxs[:, 0].max() >= X or idxs[:, 1].max() >= Y:
            raise ValueError(f'{who}: group {g} has a member outside the {X} x {Y} grid')
        members.append(idxs[:, 0].astype(np.int64) * Y + idxs[:, 1])
        offsets.append(offsets[-1] + len(idxs))
    return np.asarray(offsets, dtype=np.int64), np.concatenate(members)


def _check(data, groupings, who):
    if data.ndim != 4:
        raise ValueError(f'{who}: data must be (trials, X, Y, time), got {data.ndim} dimensions')
    for avgIdxs in groupings:
        if len(avgIdxs) == 0:
            raise ValueError(f'{who}: a grouping has no groups')
    return [_csr(data.shape, avgIdxs, who) for avgIdxs in groupings]


def spatial_avg_sweep(data, list_of_avgIdxs):
    """[spatial_avg_data(data, avgIdxs) for avgIdxs in list_of_avgIdxs] as DEVICE tensors: (trials, time, groups) float64
    contiguous views of one slab, from ONE launch that reads ``data`` once (xps_group_mean_many_*).  ``data``
    (trials, X, Y, time), float32 or float64, numpy or torch, is uploaded once if it is on the host; nothing synchronises.
    Each tensor holds the bits spatial_avg_data gives for that grouping."""
    from .._dev import stream
    from ..alignment._linalg import F64, to_device
    if len(list_of_avgIdxs) == 0:
        raise ValueError('spatial_avg_sweep: no groupings')
    csr = _check(data, list_of_avgIdxs, 'spatial_avg_sweep')
    d = to_device(data)
    N, X, Y, T = d.shape
    gstart = np.concatenate([[0], np.cumsum([len(o) - 1 for o, _ in csr])])
    mstart = np.concatenate([[0], np.cumsum([len(m) for _, m in csr])])
    offsets = np.concatenate([o[:-1] + ms for (o, _), ms in zip(csr, mstart[:-1])] + [mstart[-1:]])
    S, Gtot = len(csr), int(gstart[-1])
    meta = torch.from_numpy(np.concatenate([gstart, offsets] + [m for _, m in csr]).astype(np.int32)).to(d.device)
    slab = torch.empty(N * T * Gtot, dtype=F64, device=d.device)
    p = meta.data_ptr()
    fn = 'xps_group_mean_many_f32' if d.dtype == torch.float32 else 'xps_group_mean_many_f64'
    call(fn, d.data_ptr(), N, X * Y, T, p, p + 4 * (S + 1), p + 4 * (S + 1 + Gtot + 1), S, Gtot, slab.data_ptr(), stream())
    return [slab[N * T * int(a):N * T * int(b)].view(N, T, int(b - a)) for a, b in zip(gstart[:-1], gstart[1:])]


def spatial_avg_data(data, avgIdxs):
    """Mean of ``data`` (trials, X, Y, time) over each group of grid cells of ``avgIdxs`` -> (trials, time, groups) float64,
    the reference's bits (members added in order in the input's dtype, one division, widened).  numpy in -> numpy out, a
    device tensor in -> a device tensor out."""
    from .._dev import stream
    from ..alignment._linalg import F64, like_input, to_device
    (offsets, members), = _check(data, [avgIdxs], 'spatial_avg_data')
    d = to_device(data)
    N, X, Y, T = d.shape
    G = len(offsets) - 1
    meta = torch.from_numpy(np.concatenate([offsets, members]).astype(np.int32)).to(d.device)
    out = torch.empty(N, T, G, dtype=F64, device=d.device)
    fn = 'xps_group_mean_f32' if d.dtype == torch.float32 else 'xps_group_mean_f64'
    call(fn, d.data_ptr(), N, X * Y, T, meta.data_ptr(), meta.data_ptr() + 4 * (G + 1), G, out.data_ptr(), stream())
    return like_input(out, data)
