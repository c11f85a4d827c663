"""Realtime (streaming) CTC-RNN inference on MI355X — counterpart of the reference's
realtime_sim/realtime_nn_model.py (StackedRNN :22, DenseClassifier :66, RealtimeRNNModel :93,
forward :153, reformat_time_windows :172).  BASELINE config 5: per-step GRU inference captured in a
hipGraph.

Scope: forward with the reference's parameter names (``rnn.rnn.*``, ``h0``,
``classifier.fc.*``) so reference checkpoints load, and CTC training (training/validation/test steps,
fused CTC loss kernel, PER).

* ``forward(x)``: the right-aligned sliding windows are never materialised — window w of trial b is the
  contiguous ``win*C`` floats at ``x[b, w*stride]``, read by the input-projection GEMM through a row map;
  the recurrence runs in the fused GRU kernel with the trainable ``h0``.
* ``StreamingDecoder``: one 20 ms step (window -> L GRU cells -> Linear) recorded ONCE into a hipGraph on
  static device buffers and replayed per step; the hidden state never leaves the device.
"""
import torch
import torch.nn as nn

from ..nn_models import functional as XF
from ..nn_models._lightning import LightningModule
from .._dev import current_device, stream
from .._lib import call as _call, rowmap  # noqa: F401
from ._ctc_host import EDIT_MAX_PRED, EDIT_MAX_TARGET
from .ctc_align import forced_align
from .ctc_occupancy import posterior_align
from .ctc_decoder import greedy_decode_batch, greedy_decode_device  # noqa: F401
from .ctc_errors import edit_align


class StackedRNN(nn.Module):
    def __init__(self, input_size, hidden_size, n_layers, dropout=0.3, bidirectional=False):
        super().__init__()
        self.rnn = nn.GRU(input_size=input_size, hidden_size=hidden_size, num_layers=n_layers,
                          dropout=dropout if n_layers > 1 else 0, bidirectional=bidirectional, batch_first=True)


class DenseClassifier(nn.Module):
    def __init__(self, input_size, n_classes):
        super().__init__()
        self.fc = nn.Linear(input_size, n_classes)


def _layer_params(rnn, layer, ndir):
    out = []
    for d in range(ndir):
        sfx = f'_l{layer}' + ('_reverse' if d else '')
        out.append(tuple(getattr(rnn, n + sfx) for n in ('weight_ih', 'weight_hh', 'bias_ih', 'bias_hh')))
    return out


class _HipCTCLoss(nn.CTCLoss):
    """nn.CTCLoss whose default configuration dispatches to the fused HIP kernel.  Takes (T, B, C) log-probs as
    nn.CTCLoss does (the kernel re-normalises: a no-op on log-probabilities)."""

    def forward(self, log_probs, targets, input_lengths, target_lengths):
        if self.reduction == 'mean' and log_probs.is_cuda and log_probs.dim() == 3 and targets.dim() == 2:
            return XF.ctc_loss(log_probs, targets, input_lengths, target_lengths, blank=self.blank,
                               zero_infinity=self.zero_infinity)
        return super().forward(log_probs, targets, input_lengths, target_lengths)


def edit_distance_device(pred, pred_lengths, targets, target_lengths):
    """Levenshtein distances of B padded pairs in ONE launch (xps_edit_distance_i64), no synchronisation.  pred (B, P) /
    targets (B, L) integer device tensors with their lengths (B,) -> (B,) int64 device tensor.  ValueError beyond
    P = 65536 or L = 1024 (there is no CPU fallback)."""
    if pred.dim() != 2 or targets.dim() != 2 or pred.size(0) != targets.size(0):
        raise ValueError(f'padded pairs of shapes {tuple(pred.shape)} and {tuple(targets.shape)}: expected (B, P) and (B, L)')
    B, P, L = pred.size(0), pred.size(1), targets.size(1)
    if P > EDIT_MAX_PRED or L > EDIT_MAX_TARGET:
        raise ValueError(f'edit distance of up to {P} against {L} tokens: the kernel supports {EDIT_MAX_PRED} against '
                         f'{EDIT_MAX_TARGET}')
    if not pred.is_cuda:
        raise RuntimeError('cross_patient_speech_decoding_amd: edit_distance_device needs device tensors (no CPU fallback)')
    dev = pred.device
    pred = pred.to(torch.int64).contiguous()
    targets = targets.to(dev, torch.int64).contiguous()
    pl = torch.as_tensor(pred_lengths).to(dev, torch.int64).contiguous()
    tl = torch.as_tensor(target_lengths).to(dev, torch.int64).contiguous()
    if pl.numel() != B or tl.numel() != B:
        raise ValueError(f'{pl.numel()} / {tl.numel()} lengths for {B} pairs')
    dist = torch.empty(B, dtype=torch.int64, device=dev)
    _call('xps_edit_distance_i64', pred.data_ptr(), P, pl.data_ptr(), targets.data_ptr(), L, tl.data_ptr(), B, P, L,
          dist.data_ptr(), stream(dev))
    return dist


def per_device(tokens, lengths, targets, target_lengths):
    """Phoneme error rate in percent of a decoded batch as a 0-dim float64 DEVICE tensor (no synchronisation):
    100 * sum of edit distances / sum of target lengths (reference :307-324)."""
    dist = edit_distance_device(tokens, lengths, targets, target_lengths)
    total = torch.as_tensor(target_lengths).to(dist.device).sum().double()
    return dist.sum().double() / total * 100


_WHO = 'cross_patient_speech_decoding_amd: the edit-distance kernel'        # named by the "needs the MI355X" error


def edit_distance(a, b):
    """Levenshtein distance of two label sequences (torchaudio.functional.edit_distance), on the device."""
    dev = current_device(_WHO)
    a = torch.as_tensor([int(v) for v in a], dtype=torch.int64, device=dev).reshape(1, -1)
    b = torch.as_tensor([int(v) for v in b], dtype=torch.int64, device=dev).reshape(1, -1)
    return int(edit_distance_device(a, [a.size(1)], b, [b.size(1)])[0])


def calc_PER(decoded, targets, target_lengths):
    """Phoneme error rate in percent (reference :303-324): decoded = list of 1-D LongTensors (greedy_decode_batch)."""
    dev = current_device(_WHO)
    lengths = torch.tensor([int(p.numel()) for p in decoded], dtype=torch.int64)
    width = int(lengths.max()) if len(decoded) else 0
    tokens = torch.zeros(len(decoded), width, dtype=torch.int64, device=dev)
    for i, p in enumerate(decoded):
        tokens[i, :p.numel()] = torch.as_tensor(p).to(dev)
    targets = torch.as_tensor(targets)
    if targets.dim() == 1:
        targets = targets.reshape(len(decoded), -1)
    return float(per_device(tokens, lengths, targets.to(dev), target_lengths))


class RealtimeRNNModel(LightningModule):
    def __init__(self, input_size, hidden_size, n_layers, n_classes, dropout=0.3, win_size=14, stride=4,
                 bidirectional=False, learning_rate=1e-3, decay_steps=100, weight_decay=1e-5, blank=0):
        super().__init__()
        self.hparams_ = dict(input_size=input_size, hidden_size=hidden_size, n_layers=n_layers, n_classes=n_classes,
                             dropout=dropout, win_size=win_size, stride=stride, bidirectional=bidirectional,
                             learning_rate=learning_rate, decay_steps=decay_steps, weight_decay=weight_decay,
                             blank=blank)
        self.rnn = StackedRNN(input_size, hidden_size, n_layers, dropout, bidirectional)
        for name, param in self.rnn.named_parameters():
            if 'weight_hh' in name:
                nn.init.orthogonal_(param)
            if 'weight_ih' in name:
                nn.init.xavier_uniform_(param)
        ndir = 2 if bidirectional else 1
        self.h0 = nn.Parameter(torch.zeros(n_layers * ndir, 1, hidden_size))
        nn.init.xavier_uniform_(self.h0)
        self.classifier = DenseClassifier(hidden_size * ndir, n_classes)
        with torch.no_grad():
            self.classifier.fc.bias[:] = -2.0
            self.classifier.fc.bias[blank] = 2.0
        self.win_size, self.stride, self.blank = win_size, stride, blank
        self.criterion = _HipCTCLoss(blank=blank, zero_infinity=True)

    def n_windows(self, T):
        return (T - self.win_size) // self.stride + 1

    def forward_tm(self, x):
        """x (B, T, C) -> TIME-major logits (n_windows, B, n_classes); differentiable (weights and h0)."""
        rnn = self.rnn.rnn
        ndir = 2 if rnn.bidirectional else 1
        H, L = rnn.hidden_size, rnn.num_layers
        x = x.contiguous()
        B, T, Cc = x.shape
        nw = self.n_windows(T)
        if self.win_size * Cc != rnn.input_size:
            raise ValueError(f'input_size {rnn.input_size} != win_size * channels = {self.win_size * Cc}')
        inp = None
        for l in range(L):
            params = _layer_params(rnn, l, ndir)
            if l == 0:          # windows addressed through a row map, never materialised
                gis = [XF.WindowLinearFn.apply(x, w_ih, b_ih, self.win_size, self.stride) for w_ih, _, b_ih, _ in params]
            else:
                gis = [XF.linear(inp, w_ih, b_ih) for w_ih, _, b_ih, _ in params]
            gi = gis[0].unsqueeze(0) if ndir == 1 else torch.stack(gis, dim=0)
            h0 = self.h0[l * ndir:(l + 1) * ndir].expand(-1, B, -1).contiguous()
            y_ext = XF.GRURecurFn.apply(gi, h0, ndir, *[p[1] for p in params], *[p[3] for p in params])
            inp = y_ext[1:nw + 1]
            if l < L - 1:       # nn.GRU: dropout on the outputs of every layer but the last
                inp = XF.dropout(inp, rnn.dropout, self.training)
        return XF.linear(inp.contiguous(), self.classifier.fc.weight, self.classifier.fc.bias)     # (nw, B, C)

    def forward(self, x):
        """x (B, T, C) -> logits (B, n_windows, n_classes)  (reference :153-170)."""
        return self.forward_tm(x).permute(1, 0, 2).contiguous()

    # ---- training (reference :201-300): CTC loss on the window outputs, PER on validation -------------------
    def _adjusted_lengths(self, input_lengths):
        return ((input_lengths - self.win_size) // self.stride) + 1

    def _ctc(self, batch, adjust=True):
        inputs, targets, input_lengths, target_lengths = batch
        il = self._adjusted_lengths(input_lengths) if adjust else input_lengths
        logits_tm = self.forward_tm(inputs)
        # the fused kernel takes raw time-major scores (the log-softmax is inside): same value as
        # criterion(log_softmax(logits).permute(1, 0, 2), ...) without the (B, T, C) log-prob tensor
        loss = XF.ctc_loss(logits_tm, targets, il, target_lengths, blank=self.blank, zero_infinity=True)
        return loss, logits_tm

    def training_step(self, batch, batch_idx):
        loss, _ = self._ctc(batch)
        self.log('train_loss', loss, on_step=False, on_epoch=True, prog_bar=True)
        return loss

    def validation_step(self, batch, batch_idx):
        loss, logits_tm = self._ctc(batch)
        self.log('val_loss', loss, on_step=False, on_epoch=True, prog_bar=True)
        with torch.no_grad():       # one decode launch + one edit-distance launch; the PER stays on the device until it is read
            tokens, lengths = greedy_decode_device(logits_tm, blank=self.blank, time_major=True)   # argmax: softmax-invariant
            per = per_device(tokens, lengths, batch[1], batch[3])
            self.log('val_PER', per, on_step=False, on_epoch=True, prog_bar=True)
        return loss

    def test_step(self, batch, batch_idx):
        loss, _ = self._ctc(batch, adjust=False)           # the reference passes the raw lengths here (:283-286)
        self.log('test_loss', loss)
        return loss

    def configure_optimizers(self):
        hp = self.hparams_
        optimizer = torch.optim.AdamW(self.parameters(), lr=hp['learning_rate'], weight_decay=hp['weight_decay'])
        scheduler = torch.optim.lr_scheduler.LinearLR(optimizer, start_factor=1.0, end_factor=0.0,
                                                      total_iters=hp['decay_steps'])
        return [optimizer], [scheduler]

    def _eval_log_probs(self, x):
        """Window log-probabilities of x (B, T, C): a forward pass in eval mode under no_grad, log-softmax; the mode is put back."""
        was_training = self.training
        self.eval()
        try:
            with torch.no_grad():
                return torch.log_softmax(self.forward(x), dim=2)
        finally:
            self.train(was_training)

    def forced_align(self, x, targets, target_lengths=None):
        """x (B, T, C) with its known targets -> CTCAlignment (realtime_sim/ctc_align.py) of the targets through the model's
        own window log-probabilities: a forward pass in eval mode under no_grad, log-softmax, forced_align.  Frame w of the
        alignment is window w; window_end_times gives its time."""
        return forced_align(self._eval_log_probs(x), targets, target_lengths=target_lengths, blank=self.blank)

    def posterior_align(self, x, targets, target_lengths=None):
        """x (B, T, C) with its known targets -> CTCOccupancy (realtime_sim/ctc_occupancy.py): the forward-backward
        posteriors of the targets through the model's own window log-probabilities, by forced_align's steps.  Frame w is
        window w; log_z is -nll."""
        return posterior_align(self._eval_log_probs(x), targets, target_lengths=target_lengths, blank=self.blank)

    def decode_errors(self, x, targets, target_lengths=None, input_lengths=None):
        """x (B, T, C) with its known targets -> EditAlignment (realtime_sim/ctc_errors.py) of the model's own greedy decode
        against them: a forward pass in eval mode under no_grad, greedy_decode_device, edit_align with the model's classes,
        so .confusion is the (n_classes + 1, n_classes + 1) phoneme confusion matrix of the batch.  target_lengths None: all
        of targets' columns.  input_lengths (B,), the valid input rows of each trial (None: all T): the windows past a
        trial's adjusted length, (input_length - win_size) // stride + 1, are decoded as blank."""
        lp = self._eval_log_probs(x)
        if input_lengths is not None:
            il = torch.as_tensor(input_lengths).to(lp.device).reshape(-1, 1)
            past = torch.arange(lp.size(1), device=lp.device)[None, :] >= self._adjusted_lengths(il)
            pad = torch.full((lp.size(2),), -float('inf'), dtype=lp.dtype, device=lp.device)
            pad[self.blank] = 0.0
            lp = torch.where(past[:, :, None], pad, lp)
        tokens, lengths = greedy_decode_device(lp, blank=self.blank)
        return edit_align(tokens, lengths, targets, target_lengths, n_classes=self.classifier.fc.out_features)

    def reformat_time_windows(self, x):
        """(B, T, C) -> (B, n_windows, win*C) right-aligned windows (materialised; for inspection only)."""
        B, T, Cc = x.shape
        nw = self.n_windows(T)
        idx = (torch.arange(nw, device=x.device) * self.stride)[:, None] + torch.arange(self.win_size, device=x.device)
        return x[:, idx, :].reshape(B, nw, self.win_size * Cc)


class StreamingDecoder:
    """Per-step streaming inference replayed from a hipGraph: ``step(window)`` runs one window (win*C
    floats per stream, 1..8 streams) through all GRU layers and the classifier with the weight-streaming
    GEMV kernels (xps_gru_cell_gemv_f32: one launch per layer, xps_gemv_f32 for the classifier); the
    hidden state lives in two static device buffers that alternate between steps (two captured graphs)."""

    def __init__(self, model, n_streams=1, use_graph=True):
        from .._lib import call
        rnn = model.rnn.rnn
        if rnn.bidirectional:
            raise ValueError('streaming decode needs a unidirectional model')
        if not 1 <= n_streams <= 8:
            raise ValueError('1..8 streams per decoder')
        self.model, self.B = model, n_streams
        self.H, self.L, self.K = rnn.hidden_size, rnn.num_layers, rnn.input_size
        dev = next(model.parameters()).device
        if dev.type != 'cuda':
            raise RuntimeError('StreamingDecoder needs the model on the GPU (no CPU fallback)')
        self.dev, self._call = dev, call
        S = 1 << (n_streams - 1).bit_length()                 # rows allocated: power of two >= B
        self.n_classes = model.classifier.fc.out_features
        self.window = torch.zeros(S, self.K, dtype=torch.float32, device=dev)
        self.hbuf = torch.zeros(2, self.L, S, self.H, dtype=torch.float32, device=dev)    # ping-pong state
        self._logits = torch.zeros(S, self.n_classes, dtype=torch.float32, device=dev)
        self._token = torch.zeros(S, dtype=torch.int64, device=dev)
        self._params = [tuple(p.detach().contiguous() for p in _layer_params(rnn, l, 1)[0]) for l in range(self.L)]
        self._fc = (model.classifier.fc.weight.detach().contiguous(), model.classifier.fc.bias.detach().contiguous())
        self.parity = 0
        self.graphs = None
        self.reset()
        if use_graph:
            for par in (0, 1):                                # warm-up: module load, allocator
                self._body(par)
            torch.cuda.synchronize()
            self.graphs = []
            for par in (0, 1):
                g = torch.cuda.CUDAGraph()
                with torch.cuda.graph(g):
                    self._body(par)
                self.graphs.append(g)
            self.reset()

    @property
    def logits(self):
        return self._logits[:self.B]

    @property
    def token(self):
        return self._token[:self.B]

    @property
    def h(self):
        return self.hbuf[self.parity, :, :self.B]

    def reset(self):
        with torch.no_grad():
            self.hbuf.zero_()
            self.hbuf[:, :, :self.B] = self.model.h0.detach().expand(-1, self.B, -1)
        self.parity = 0

    @torch.no_grad()
    def _body(self, par):
        st = stream()
        src, dst = self.hbuf[par], self.hbuf[par ^ 1]
        inp, k = self.window, self.K
        for l, (w_ih, w_hh, b_ih, b_hh) in enumerate(self._params):
            self._call('xps_gru_cell_gemv_f32', inp.data_ptr(), k, w_ih.data_ptr(), w_hh.data_ptr(), b_ih.data_ptr(),
                       b_hh.data_ptr(), src[l].data_ptr(), dst[l].data_ptr(), self.H, self.B, st)
            inp, k = dst[l], self.H
        self._call('xps_gemv_f32', inp.data_ptr(), self._fc[0].data_ptr(), self._fc[1].data_ptr(), self._logits.data_ptr(),
                   self.n_classes, self.H, self.B, st)
        self._call('xps_next_token', self._logits.data_ptr(), self.n_classes, None, 0, None, self._token.data_ptr(),
                   self.B, st)

    @torch.no_grad()
    def step(self, window=None):
        """window: (n_streams, win*C) device or host tensor (None: reuse the static buffer).  Returns the
        logits (n_streams, n_classes) in a static buffer; ``self.token`` holds the argmax class."""
        if window is not None:
            self.window[:self.B].copy_(window.reshape(self.B, self.K), non_blocking=True)
        if self.graphs is not None:
            self.graphs[self.parity].replay()
        else:
            self._body(self.parity)
        self.parity ^= 1
        return self.logits
