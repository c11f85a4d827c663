"""Per-bin high-gamma feature extraction on the MI355X — counterpart of the reference's
realtime_sim/realtime_processing.py (process_HG :10, CAR :42, filter_HG_bin :60, FIR_filter_HG_bin :86,
IIR_filter_HG_bin :106, compute_bin_power :146): same names, arguments and return values (numpy float64).

Every function is one launch of the fused HIP kernel (xps_process_hg_f64: common average reference -> band-pass filters
with carried state -> RMS); ``process_HG`` runs all three stages in a single launch and
``process_HG_trials`` runs them over every bin of N recorded trials in one launch (xps_hg_trials_f64), bit for bit what
looping ``process_HG`` over a trial's bins gives.  The IIR path reproduces
scipy.signal.lfilter's direct-form-II-transposed arithmetic bit for bit (no fused multiply-add), the CAR and RMS stages
numpy's summation order; the FIR path (scipy evaluates it with np.convolve / BLAS dot products, whose summation order
is not defined) agrees to rounding.  There is no CPU fallback."""

import numpy as np
import torch

from .._dev import current_device, ptr, stream, workspace
from .._lib import call, lib

_F64 = torch.float64
_WHO = 'realtime_processing'        # named by the "needs the MI355X" error


def _up(x):
    if x is None:
        return None
    return torch.as_tensor(np.ascontiguousarray(x, dtype=np.float64)).to(current_device(_WHO))


def lfilter_zi(b, a):
    """scipy.signal.lfilter_zi: steady-state filter state of a unit step (companion-matrix solve; float64)."""
    b, a = np.atleast_1d(np.asarray(b, dtype=np.float64)), np.atleast_1d(np.asarray(a, dtype=np.float64))
    while len(a) > 1 and a[0] == 0.0:
        a = a[1:]
    if a[0] != 1.0:
        b, a = b / a[0], a / a[0]
    n = max(len(a), len(b))
    a = np.r_[a, np.zeros(n - len(a))]
    b = np.r_[b, np.zeros(n - len(b))]
    comp = np.zeros((n - 1, n - 1))
    comp[0, :] = -a[1:] / a[0]
    comp[np.arange(1, n - 1), np.arange(0, n - 2)] = 1.0
    return np.linalg.solve(np.eye(n - 1) - comp.T, b[1:] - a[1:] * b[0])


def _run(data, b=None, a=None, zi=None, good=None, do_car=True, want='power'):
    """One launch.  ``want``: 'car' | 'filtered' | 'power'.  Returns (result ndarray, updated zi ndarray or None)."""
    data = np.asarray(data, dtype=np.float64)
    Cn, Tn = data.shape
    dev = current_device(_WHO)
    d = _up(data)
    bands = 0 if b is None else b.shape[0]
    taps = 1 if b is None else b.shape[1]
    bd, ad = _up(b), _up(a)
    zd = _up(zi)
    gd = None if good is None else torch.as_tensor(np.ascontiguousarray(good, dtype=np.uint8)).to(dev)
    car = torch.empty(Cn, Tn, dtype=_F64, device=dev) if want == 'car' else None
    filt = torch.empty(Cn, Tn, max(bands, 1), dtype=_F64, device=dev) if want == 'filtered' else None
    power = torch.empty(Cn, dtype=_F64, device=dev) if want == 'power' else None
    nbytes = lib().xps_process_hg_f64_workspace(Cn, Tn, max(bands, 1))
    ws = workspace(nbytes, dev)
    call('xps_process_hg_f64', ptr(d), Cn, Tn, ptr(gd), ptr(bd), ptr(ad), bands, taps, ptr(zd), int(do_car), ptr(car),
         ptr(filt), ptr(power), ptr(ws), nbytes, stream())
    out = car if want == 'car' else (filt if want == 'filtered' else power)
    return out.cpu().numpy(), (None if zd is None else zd.cpu().numpy())


def _good_mask(n_chan, bad_channels):
    good = np.ones(n_chan, dtype=np.uint8)
    for c in (bad_channels or []):
        good[c] = 0
    return good


def _split_coefs(bandpassCoefs, n_chan, band_ics):
    """(b, a, zi) arrays for the kernel from the reference's coefficient layouts."""
    coefs = np.asarray(bandpassCoefs, dtype=np.float64)
    if coefs.ndim == 3:                              # IIR: (bands, taps, [a, b])
        a, b = np.ascontiguousarray(coefs[:, :, 0]), np.ascontiguousarray(coefs[:, :, 1])
        if band_ics is None:                         # :129-136: lfilter_zi tiled over the channels
            zi = np.stack([np.tile(lfilter_zi(bb, aa), (n_chan, 1)) for bb, aa in zip(b, a)], axis=0)
        else:
            zi = np.asarray(band_ics, dtype=np.float64)
        return b, a, zi
    if coefs.ndim == 2:                              # FIR: (bands, taps); lfilter(coefs, 1.0, data): zero state, not returned
        return np.ascontiguousarray(coefs), None, None
    raise ValueError('bandpassCoefs must be either 2D or 3D array.')


def CAR(data, bad_channels=None):
    """Common average reference (reference :42-57)."""
    data = np.asarray(data, dtype=np.float64)
    out, _ = _run(data, good=_good_mask(data.shape[0], bad_channels), do_car=True, want='car')
    return out


def IIR_filter_HG_bin(data, bandpassCoefs, zi=None):
    """(channels, time) -> ((channels, time, bands), (bands, channels, order)) (reference :106-143)."""
    data = np.asarray(data, dtype=np.float64)
    b, a, z = _split_coefs(bandpassCoefs, data.shape[0], zi)
    return _run(data, b, a, z, do_car=False, want='filtered')


def FIR_filter_HG_bin(data, bandpassCoefs):
    """(channels, time) -> ((channels, time, bands), None) (reference :86-103)."""
    data = np.asarray(data, dtype=np.float64)
    b, _, _ = _split_coefs(bandpassCoefs, data.shape[0], None)
    out, _ = _run(data, b, None, None, do_car=False, want='filtered')
    return out, None


def filter_HG_bin(data, bandpassCoefs, band_ics=None):
    """Routes to the IIR (3-D coefficients) or FIR (2-D) filter (reference :60-83)."""
    bandpassCoefs = np.asarray(bandpassCoefs)
    if bandpassCoefs.ndim == 3:
        return IIR_filter_HG_bin(data, bandpassCoefs, band_ics)
    if bandpassCoefs.ndim == 2:
        return FIR_filter_HG_bin(data, bandpassCoefs)
    raise ValueError('bandpassCoefs must be either 2D or 3D array.')


def compute_bin_power(data):
    """RMS over (time, bands) per channel of a (channels, time, bands) array (reference :146-164)."""
    data = np.asarray(data, dtype=np.float64)
    Cn, Tn, nb = data.shape
    # the kernel's identity "filter" (one tap, b = 1) over the flattened (time*bands) samples as ONE band keeps the
    # contiguous summation order np.mean(axis=(1, 2)) uses
    out, _ = _run(data.reshape(Cn, Tn * nb), np.ones((1, 1)), None, None, do_car=False, want='power')
    return out


def process_HG(data, bandpassCoefs, bad_channels=None, filt_ics=None):
    """CAR -> band-pass -> RMS band power in ONE launch (reference :10-39).  Returns (power (channels,), filt_ics)."""
    data = np.asarray(data, dtype=np.float64)
    b, a, z = _split_coefs(bandpassCoefs, data.shape[0], filt_ics)
    return _run(data, b, a, z, good=_good_mask(data.shape[0], bad_channels), do_car=True, want='power')


def _hg_trials(raw, b, a, bands, taps, lengths=None, good=None, zi=None, want_state=False, want_power=True,
               fmap=None, map_of_trial=None, n_maps=0):
    """One xps_hg_trials_f64 launch on device tensors, no synchronisation.  raw (N, n_bins, C, Tn) float32 / float64
    contiguous; b, a (bands, taps) float64 (a None: FIR); lengths (N,) int64 or None; good (C,) or (N, C) uint8 or None;
    zi (bands, C, taps-1) or (N, bands, C, taps-1) or None; fmap None (no features), (None, None, d) for the identity
    cast or (W (n_maps, C, d), c (n_maps, d) or None, d); map_of_trial (N,) int32 or None, checked by the kernel against
    n_maps (W's, or the argument under the identity map): a trial with an index outside gets NaN features.
    Returns (power or None, state or None, features or None)."""
    N, n_bins, Cn, Tn = raw.shape
    dev = raw.device
    power = torch.empty(N, n_bins, Cn, dtype=_F64, device=dev) if want_power else None
    state = torch.empty(N, bands, Cn, taps - 1, dtype=_F64, device=dev) if want_state else None
    W = c = feats = None
    d = 0
    if fmap is not None:
        W, c, d = fmap
        n_maps = n_maps if W is None else W.shape[0]
        feats = torch.empty(N, n_bins, d, dtype=torch.float32, device=dev)
    nbytes = int(lib().xps_hg_trials_f64_workspace(N, n_bins, Cn, Tn, bands))
    ws = workspace(nbytes, dev)
    call('xps_hg_trials_f64', raw.data_ptr(), int(raw.dtype == torch.float32), N, n_bins, Cn, Tn, ptr(lengths), ptr(good),
         int(good is not None and good.dim() == 2), ptr(b), ptr(a), bands, taps, ptr(zi), int(zi is not None and zi.dim() == 4),
         ptr(state), ptr(power), ptr(W), ptr(c), ptr(map_of_trial), n_maps, d, ptr(feats), ws.data_ptr(), nbytes,
         stream(dev))
    return power, state, feats


def _check_trials(data, n_chan=None, bin_samples=None):
    """(N, n_bins, C, Tn) tensor with no empty axis (and the given C, Tn), or ValueError with the shape."""
    data = torch.as_tensor(data)
    if data.dim() != 4 or 0 in data.shape or (n_chan is not None and (data.shape[2], data.shape[3]) != (n_chan, bin_samples)):
        want = '(N, n_bins, n_channels, bin_samples)' if n_chan is None else f'(N, n_bins, {n_chan}, {bin_samples})'
        raise ValueError(f'trials of shape {tuple(data.shape)}: expected {want}, no empty axis')
    return data


def _trials_on_device(data, n_chan=None, bin_samples=None):
    """Checked trials, host or device, float32 or float64 (anything else is widened to float64) -> contiguous device tensor."""
    data = _check_trials(data, n_chan, bin_samples)
    if data.dtype not in (torch.float32, torch.float64):
        data = data.to(_F64)
    return data.to(current_device(_WHO)).contiguous()


def _trial_lengths(lengths, N, n_bins):
    """lengths (N,) -> host int64 tensor, checked against 0..n_bins (None stays None)."""
    if lengths is None:
        return None
    lens = torch.as_tensor(lengths).to('cpu', torch.int64).reshape(-1)
    if lens.numel() != N:
        raise ValueError(f'lengths of shape {tuple(torch.as_tensor(lengths).shape)} for {N} trials')
    if int(lens.min()) < 0 or int(lens.max()) > n_bins:
        raise ValueError(f'lengths outside 0..{n_bins}')
    return lens


def process_HG_trials(data, bandpassCoefs, bad_channels=None, filt_ics=None, lengths=None, return_state=False):
    """process_HG over every bin of N trials in ONE launch: data (N, n_bins, channels, time) host or device, float32 or
    float64 -> device float64 (N, n_bins, channels); row j of trial n is process_HG of that bin with the filter state bin
    j - 1 left (bin 0: ``filt_ics`` (bands, channels, order), or one per trial (N, bands, channels, order); default
    lfilter_zi tiled over the channels).  ``lengths`` (N,): trial n has that many bins, the rows after them are zeros.
    ``return_state``: also the state after each trial's last bin, (N, bands, channels, order) (None for FIR).  The data
    makes no host round trip."""
    data = _check_trials(data)
    N, n_bins, Cn, _ = data.shape
    b, a, zi = _split_coefs(bandpassCoefs, Cn, filt_ics)
    bands, taps = b.shape
    if a is not None and zi.shape not in ((bands, Cn, taps - 1), (N, bands, Cn, taps - 1)):
        raise ValueError(f'filt_ics of shape {zi.shape}: expected {(bands, Cn, taps - 1)} or {(N, bands, Cn, taps - 1)}')
    lens = _trial_lengths(lengths, N, n_bins)
    raw = _trials_on_device(data)
    dev = raw.device
    good = torch.from_numpy(_good_mask(Cn, bad_channels)).to(dev)
    power, state, _ = _hg_trials(raw, _up(b), _up(a), bands, taps, None if lens is None else lens.to(dev), good,
                                 None if a is None else _up(zi), want_state=return_state and a is not None)
    return (power, state) if return_state else power
