"""Sliding-window sub-grids of an electrode array (reference processing_utils/grid_subsampling.py).

Index generation stays on the host: it is tiny and it defines the order of everything downstream.  What the subsample scripts do
with the index lists -- slice channel-last features as X[:, :, idx] once per window -- is select_channels_sweep: every
window of a sweep from ONE launch that reads the resident features once (xps_select_channels_*)."""
import numpy as np
import torch

from .._lib import call


def _load_mat(dataPath, pt, name, key):
    import scipy.io as sio
    return sio.loadmat(f'{dataPath}/{pt}/{pt}_{name}.mat')[key]


def _trimmed_chan_map(pt, dataPath, chanMap):
    """The patient's channel map with the all-NaN border of a 24-wide side cut off; also which side it was (0, 1 or None)."""
    chanMap = _load_mat(dataPath, pt, 'channelMap', 'chanMap') if chanMap is None else np.asarray(chanMap)
    if chanMap.shape[0] == 24:
        return chanMap[1:-1, :], 0
    if chanMap.shape[1] == 24:
        return chanMap[:, 1:-1], 1
    return chanMap, None


def _sig_channels(pt, dataPath, sigChannel):
    sig = _load_mat(dataPath, pt, 'sigChannel', 'sigChannel') if sigChannel is None else np.asarray(sigChannel)
    return np.squeeze(sig)


def grid_susbsample_idxs(gridSize, winSize, step=(1, 1), start=(0, 0)):
    """(row, col) index arrays, each (winSize[0] * winSize[1], 2), of every position of a winSize window on a gridSize grid.

    Order (the reference's meshgrid order): window positions with the row start running fastest; inside a window the row
    index runs fastest."""
    d_row = np.tile(np.arange(winSize[0]), winSize[1])
    d_col = np.repeat(np.arange(winSize[1]), winSize[0])
    rows = np.arange(start[0], gridSize[0] - winSize[0] + 1, step[0])
    cols = np.arange(start[1], gridSize[1] - winSize[1] + 1, step[1])
    return [np.stack([r + d_row, c + d_col], axis=1) for c in cols for r in rows]


def grid_subsample_sig_channels(pt, winSize, dataPath, step=(1, 1), *, chanMap=None, sigChannel=None):
    """Per sliding window: positions, inside the patient's significant-channel list, of the significant channels the window
    samples; windows without one are left out.  ``chanMap`` / ``sigChannel`` arrays replace
    {dataPath}/{pt}/{pt}_channelMap.mat and {pt}_sigChannel.mat (nothing is read from disk for an argument that is given)."""
    chanMap, trimmed = _trimmed_chan_map(pt, dataPath, chanMap)
    sig = _sig_channels(pt, dataPath, sigChannel)
    if trimmed == 0:                                  # the 24-wide side is the first one: the window is given transposed
        winSize = (winSize[1], winSize[0])
    found = []
    for idxs in grid_susbsample_idxs(chanMap.shape, winSize, step=step):
        elec = chanMap[idxs[:, 0], idxs[:, 1]]
        elec = elec[~np.isnan(elec)].astype(int)      # non-rectangular maps have NaN cells
        where = np.intersect1d(sig, elec, return_indices=True)[1]
        if len(where) > 0:
            found.append(where)
    return found


def select_channels_sweep(X, list_of_index_arrays):
    """[X[:, :, idx] for idx in list_of_index_arrays] for channel-last features X (N, T, C), float32 or float64, numpy or
    torch, host or device: a list of (N, T, len(idx)) DEVICE tensors, contiguous views of one slab, written by one launch
    that reads X once.  X is uploaded once; nothing synchronises.  ValueError (before any launch) for an empty list, an
    empty index array, an index outside [0, C) or X.ndim != 3."""
    from .._dev import stream
    from ..alignment._linalg import to_device
    if X.ndim != 3:
        raise ValueError(f'select_channels_sweep: X must be (trials, time, channels), got {X.ndim} dimensions')
    if len(list_of_index_arrays) == 0:
        raise ValueError('select_channels_sweep: no index arrays')
    C = int(X.shape[2])
    lists = [np.asarray(i).reshape(-1) for i in list_of_index_arrays]
    for s, i in enumerate(lists):
        if i.size == 0:
            raise ValueError(f'select_channels_sweep: index array {s} is empty')
        if not np.issubdtype(i.dtype, np.integer) or i.min() < 0 or i.max() >= C:
            raise ValueError(f'select_channels_sweep: index array {s} has an entry outside [0, {C})')
    start = np.concatenate([[0], np.cumsum([i.size for i in lists])])
    Xd = to_device(X)
    N, T, _ = Xd.shape
    meta = torch.from_numpy(np.concatenate([start] + lists).astype(np.int32)).to(Xd.device)
    S, Ltot = len(lists), int(start[-1])
    slab = torch.empty(N * T * Ltot, dtype=Xd.dtype, device=Xd.device)
    fn = 'xps_select_channels_f32' if Xd.dtype == torch.float32 else 'xps_select_channels_f64'
    call(fn, Xd.data_ptr(), N, T, C, meta.data_ptr(), meta.data_ptr() + 4 * (S + 1), S, Ltot, slab.data_ptr(), stream())
    return [slab[N * T * int(a):N * T * int(b)].view(N, T, int(b - a)) for a, b in zip(start[:-1], start[1:])]
