"""Per-trial augmentations of the CTC data modules -- same names, arguments and random draws as the reference's
realtime_sim/augmentations.py (time_warping :14, time_masking :37, time_shifting :52, noise_jitter :64, scaling :78): ONE
draw per trial, made with the reference's generator calls in the reference's order and shapes (``draw_*`` below), applied by
the HIP kernels of csrc/xps_ctc_data.hip (jitter: xps_aug_jitter_f32).

time_warping, time_shifting and scaling draw on ``data.device``, time_masking with ``torch.randint`` on the CPU, noise_jitter
with ``randn_like``: a host tensor under ``torch.manual_seed`` therefore gets the reference's draws.  A host tensor is
uploaded, augmented and returned on the host; a device tensor stays on the device.  There is no CPU fallback.

Extensions (keywords): ``out=``, a float32 device tensor of the input's shape that receives the result -- for instance a
slab of the concatenated training tensor (the data modules write every augmented copy in place that way) -- and
``draw_device=``, the device whose generator makes the draws instead of ``data.device`` (the data modules pass 'cpu': the
reference's setup() augments host tensors, so its draws come from the CPU generator although the pooled tensor lives in HBM).

Precision: float32, the dtype the data modules hold (a float64 input is rounded, augmented and cast back).  The whole-batch
augmentations of nn_models/data_utils/augmentations.py (one draw per call) are a different family and are untouched."""
import torch

from .._dev import need_gpu, ptr, stream
from .._lib import call


# ---- the draws (host logic only: testable without the device) ------------------------------------------------------------
def draw_warp_lengths(B, T, device, factor_range=(0.8, 1.2)):
    """(factors (B,) float32, T2 (B,) int64): T2[n] = int(T * factors[n]) -- a float32 product, then truncation (:19-24)."""
    factors = torch.empty(B, device=device).uniform_(*factor_range)
    return factors, (T * factors).to(torch.int64)


def draw_mask_starts(B, T, mask_ratio=0.1):
    """(starts (B,) int64 on the CPU, mask_size) (:42-45)."""
    mask_size = int(T * mask_ratio)
    return torch.randint(0, T - mask_size + 1, (B,)), mask_size


def draw_shifts(B, device, shift_max=20):
    """shifts (B,) int64 on ``device`` (:57)."""
    return torch.randint(-shift_max, shift_max + 1, (B,), device=device)


def draw_scales(B, device, scale_range=(0.9, 1.1)):
    """scales (B, 1, 1) float32 on ``device`` (:89)."""
    return torch.empty(B, 1, 1, device=device).uniform_(*scale_range)


# ---- plumbing ------------------------------------------------------------------------------------------------------------
def _on_device(data, out):
    if not torch.is_tensor(data):
        data = torch.as_tensor(data)
    if data.dim() != 3:
        raise ValueError('augmentations expect (n_trials, n_timepoints, n_features) tensors')
    host = not data.is_cuda
    if host and not torch.cuda.is_available():
        raise RuntimeError('cross_patient_speech_decoding_amd: the augmentation kernels need the MI355X (no CPU fallback)')
    x = data.to('cuda', dtype=torch.float32).contiguous()
    need_gpu(x)
    if out is None:
        res = torch.empty_like(x)
    else:
        if not (torch.is_tensor(out) and out.is_cuda and out.dtype == torch.float32 and out.shape == x.shape
                and out.is_contiguous()):
            raise ValueError('out= must be a contiguous float32 device tensor of the input\'s shape')
        res = out
    return x, res, host, data.dtype


def _back(res, out, host, dtype):
    if out is not None:
        return out
    res = res if dtype == torch.float32 else res.to(dtype)
    return res.cpu() if host else res


def _dev(t, like, dtype):
    return t.to(like.device, dtype=dtype).contiguous()


# ---- the reference's five functions ---------------------------------------------------------------------------------------
def time_warping(data, factor_range=(0.8, 1.2), out=None, draw_device=None):
    """data (B, T, F): every trial linearly resampled to int(T * factor) samples and back to T (F.interpolate, mode='linear',
    align_corners=False, twice), one factor per trial, in one fused kernel."""
    data = torch.as_tensor(data)
    B, T, _ = data.shape
    _, T2 = draw_warp_lengths(B, T, draw_device or data.device, factor_range)
    x, res, host, dt = _on_device(data, out)
    if B and int(T2.min()) < 1:
        raise ValueError('time_warping: a warp factor gives an empty intermediate sequence')
    call('xps_aug_trial_warp_f32', ptr(x), ptr(res), B, T, x.shape[2], ptr(_dev(T2, x, torch.int64)), stream())
    return _back(res, out, host, dt)


def time_masking(data, mask_ratio=0.1, out=None, draw_device=None):
    """data (B, T, F): int(T * mask_ratio) consecutive samples zeroed, one start per trial."""
    data = torch.as_tensor(data)
    B, T, _ = data.shape
    starts, mask_size = draw_mask_starts(B, T, mask_ratio)
    x, res, host, dt = _on_device(data, out)
    call('xps_aug_trial_mask_f32', ptr(x), ptr(res), B, T, x.shape[2], ptr(_dev(starts, x, torch.int64)), int(mask_size),
         stream())
    return _back(res, out, host, dt)


def time_shifting(data, shift_max=20, out=None, draw_device=None):
    """data (B, T, F): every trial rolled along time by its own shift in [-shift_max, shift_max]."""
    data = torch.as_tensor(data)
    B, T, _ = data.shape
    shifts = draw_shifts(B, draw_device or data.device, shift_max)
    x, res, host, dt = _on_device(data, out)
    call('xps_aug_trial_shift_f32', ptr(x), ptr(res), B, T, x.shape[2], ptr(_dev(shifts, x, torch.int64)), stream())
    return _back(res, out, host, dt)


def noise_jitter(data, noise_level=0.01, out=None, draw_device=None):
    """data + N(0, 1) * noise_level (two roundings, as the reference's expression)."""
    data = torch.as_tensor(data)
    noise = torch.randn_like(data) if draw_device is None else torch.randn(data.shape, dtype=data.dtype, device=draw_device)
    x, res, host, dt = _on_device(data, out)
    nz = _dev(noise, x, torch.float32)
    call('xps_aug_jitter_f32', ptr(x), ptr(nz), ptr(res), x.numel(), float(noise_level), stream())
    return _back(res, out, host, dt)


def scaling(data, scale_range=(0.9, 1.1), out=None, draw_device=None):
    """data (B, T, F): every trial multiplied by its own uniform factor."""
    data = torch.as_tensor(data)
    B = data.size(0)
    scales = draw_scales(B, draw_device or data.device, scale_range)
    x, res, host, dt = _on_device(data, out)
    call('xps_aug_trial_scale_f32', ptr(x), ptr(res), B, x.shape[1] * x.shape[2], ptr(_dev(scales.reshape(-1), x, torch.float32)),
         stream())
    return _back(res, out, host, dt)


for _f in (time_warping, time_masking, time_shifting, noise_jitter, scaling):
    _f.writes_out = True           # the data modules hand these a slab of the training tensor through out=
