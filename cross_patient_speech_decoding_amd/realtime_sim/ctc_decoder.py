"""CTC decoding — counterpart of the reference's realtime_sim/ctc_decoder.py.

greedy_decode_batch (ctc_decoder.py:172-189, the decoder the scripts import: scripts/train_ctc_rnn.py:26): collapse repeats,
drop blanks.  decode / beam_decode_torch / beam_decode_batch: the prefix beam search of decode (ctc_decoder.py:46-118) on the
device in fp64, one workgroup per sequence (csrc/xps_ctc_beam.hip); same prefixes, same tie order.  There
is no CPU fallback."""
import numpy as np
import torch

from .._dev import ptr, stream, workspace
from .._lib import call, lib

BEAM_MAX, CLASSES_MAX, CANDIDATES_MAX = 128, 64, 8192


def greedy_decode_device(scores, blank=0, time_major=False):
    """Greedy CTC decode of a whole batch in ONE launch (xps_ctc_greedy_decode), no synchronisation.  scores: device tensor
    (B, T, C), or (T, B, C) with time_major -- any strides over the first two axes (a permuted view is read in place),
    float32 / float64 logits or log-probabilities.  Every frame is decoded.  Returns device tensors (tokens (B, T) int64:
    the decoded labels of each sequence, then -1; lengths (B,) int64)."""
    if scores.dim() != 3:
        raise ValueError(f'scores of shape {tuple(scores.shape)}: expected three axes')
    if not scores.is_cuda:
        raise RuntimeError('cross_patient_speech_decoding_amd: greedy_decode_device needs a device tensor (no CPU fallback)')
    if scores.dtype not in (torch.float32, torch.float64):
        scores = scores.float() if scores.is_floating_point() else scores.double()
    if scores.size(2) > 1 and scores.stride(2) != 1:
        scores = scores.contiguous()
    (T, B) = (scores.size(0), scores.size(1)) if time_major else (scores.size(1), scores.size(0))
    st, sb = (scores.stride(0), scores.stride(1)) if time_major else (scores.stride(1), scores.stride(0))
    Cn = scores.size(2)
    if Cn < 1:
        raise ValueError('greedy decode needs at least one class')
    tokens = torch.empty(B, T, dtype=torch.int64, device=scores.device)
    lengths = torch.empty(B, dtype=torch.int64, device=scores.device)
    call('xps_ctc_greedy_decode', scores.data_ptr(), int(scores.dtype == torch.float32), int(st), int(sb), T, B, Cn, int(blank),
         tokens.data_ptr(), lengths.data_ptr(), stream(scores.device))
    return tokens, lengths


def greedy_decode_batch(log_probs, blank=0):
    """log_probs (B, T, C) -> list of 1-D LongTensors (on the input's device).  A device tensor is decoded by the batched
    kernel (one launch, one transfer of the B lengths); a host tensor by the reference's expression."""
    if log_probs.is_cuda:
        tokens, lengths = greedy_decode_device(log_probs, blank=blank)
        return [tokens[b, :n] for b, n in enumerate(lengths.tolist())]
    best = log_probs.argmax(dim=2)
    keep = torch.ones_like(best, dtype=torch.bool)
    keep[:, 1:] = best[:, 1:] != best[:, :-1]
    keep &= best != blank
    return [best[b][keep[b]] for b in range(best.size(0))]


def check_beam_sizes(beam_size, n_classes, blank):
    """ValueError unless the beam kernels support the sizes (include/xps.h)."""
    if not 1 <= beam_size <= BEAM_MAX:
        raise ValueError(f'beam_size {beam_size} outside 1..{BEAM_MAX}')
    if not 1 <= n_classes <= CLASSES_MAX:
        raise ValueError(f'{n_classes} classes outside 1..{CLASSES_MAX}')
    if beam_size * n_classes > CANDIDATES_MAX:
        raise ValueError(f'beam_size * n_classes = {beam_size * n_classes} > {CANDIDATES_MAX}')
    if not 0 <= blank < n_classes:
        raise ValueError(f'blank {blank} outside 0..{n_classes - 1}')


def _beam_device(log_probs, input_lengths, beam_size, blank, from_logits):
    """(B, T, S) float32 / float64 tensor -> device (prefix (B, T) int64, length (B,) int64, nll (B,) float64)."""
    if log_probs.dim() != 3:
        raise ValueError(f'log_probs of shape {tuple(log_probs.shape)}: expected (B, T, n_classes)')
    B, T, S = log_probs.shape
    check_beam_sizes(int(beam_size), int(S), int(blank))
    lens = None
    if input_lengths is not None:
        lens = torch.as_tensor(input_lengths, dtype=torch.int64).reshape(-1)
        if lens.numel() != B:
            raise ValueError(f'{lens.numel()} input_lengths for {B} sequences')
        if B and (int(lens.min()) < 0 or int(lens.max()) > T):
            raise ValueError(f'input_lengths outside 0..{T}')
    if log_probs.dtype not in (torch.float32, torch.float64):
        log_probs = log_probs.double()
    dev = log_probs.device if log_probs.is_cuda else torch.device('cuda', torch.cuda.current_device())
    x = log_probs.to(dev).contiguous()
    lens = None if lens is None else lens.to(dev)
    prefix = torch.empty(B, T, dtype=torch.int64, device=dev)
    plen = torch.empty(B, dtype=torch.int64, device=dev)
    nll = torch.empty(B, dtype=torch.float64, device=dev)
    ws_bytes = int(lib().xps_ctc_beam_workspace(B, T, int(beam_size), S))
    ws = workspace(max(ws_bytes, 1), dev)
    call('xps_ctc_beam_f64', x.data_ptr(), int(x.dtype == torch.float32), B, T, S,
         ptr(lens), int(blank), int(beam_size), int(bool(from_logits)), prefix.data_ptr(),
         plen.data_ptr(), nll.data_ptr(), ws.data_ptr(), ws_bytes, stream(dev))
    return prefix, plen, nll


def beam_decode_batch(log_probs, input_lengths=None, beam_size=100, blank=0, from_logits=False, return_nll=False):
    """Batched prefix beam search, the counterpart of greedy_decode_batch.  log_probs (B, T, C) float32 / float64
    log-probabilities (from_logits: raw logits, fp64 log-softmax per row first), input_lengths (B,) or None (all T) ->
    list of 1-D LongTensors on the input's device (+ nll (B,) float64 with return_nll).  One launch for the batch."""
    log_probs = torch.as_tensor(log_probs)
    prefix, plen, nll = _beam_device(log_probs, input_lengths, beam_size, blank, from_logits)
    prefix, plen, nll = prefix.to(log_probs.device), plen.tolist(), nll.to(log_probs.device)
    out = [prefix[b, :n] for b, n in enumerate(plen)]
    return (out, nll) if return_nll else out


def _decode_one(lp, beam_size, blank):
    prefix, plen, nll = _beam_device(lp.unsqueeze(0), None, beam_size, blank, False)
    n = int(plen[0])
    return tuple(int(v) for v in prefix[0, :n].tolist()), float(nll[0])


def decode(probs, beam_size=100, blank=0):
    """The reference's decode: probs (T, S) posteriors -> (prefix tuple, nll) of the prefix beam search over log(probs)."""
    probs = np.asarray(probs.cpu() if torch.is_tensor(probs) else probs, dtype=np.float64)
    if probs.ndim != 2:
        raise ValueError(f'probs of shape {probs.shape}: expected (T, n_classes)')
    with np.errstate(divide='ignore', invalid='ignore'):
        lp = np.log(probs)
    return _decode_one(torch.from_numpy(np.ascontiguousarray(lp)), beam_size, blank)


def beam_decode_torch(probs, beam_size=100, blank=0):
    """The reference's beam_decode_torch: probs (T, S) log-probabilities (after log_softmax) -> (prefix tuple, nll), in fp64."""
    probs = torch.as_tensor(probs)
    if probs.dim() != 2:
        raise ValueError(f'probs of shape {tuple(probs.shape)}: expected (T, n_classes)')
    return _decode_one(probs.double(), beam_size, blank)
