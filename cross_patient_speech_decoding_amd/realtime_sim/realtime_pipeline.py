"""Realtime CTC pipeline on the MI355X: raw ECoG bins of one or more patients -> high-gamma power -> alignment map ->
sliding window -> GRU step -> greedy (or prefix beam search) CTC tokens, one hipGraph replay per prediction.

The reference runs these stages as separate host steps (realtime_sim/realtime_processing.py process_HG per bin, the
PCA / CCA transforms of realtime_datamodule.py, the windowing of realtime_nn_model.py and ctc_decoder.py's greedy
decode).  Here one prediction is a linear chain of launches on one stream, captured once per parity:

    xps_pipe_frontend_f64   stride bins x n_streams: CAR -> band-pass with carried state -> RMS (bit-exact process_HG)
    xps_window_shift_f32    float32(power @ W + c) shifted into the stream's window (ping-pong pair of windows)
    xps_gru_cell_gemv_f32   x L (ping-pong hidden state, as StreamingDecoder)
    xps_gemv_f32            classifier
    xps_ctc_collapse_f32    argmax + online greedy collapse into a device token buffer
    xps_ctc_beam_step_f32   decoder='beam' only: one frame of the prefix beam search, beam kept in device state

Streams are different patients sharing one model: each has its own bad channels, alignment map and filter state; a patient
with fewer electrodes is padded with bad channels and zero map rows.  There is no CPU fallback."""
import numpy as np
import torch

from .._dev import ptr, stream, workspace
from .._lib import call, lib
from .ctc_decoder import check_beam_sizes
from .realtime_nn_model import _layer_params
from .realtime_processing import _good_mask, _split_coefs

_F64 = torch.float64


def _stage_affine(st):
    """One transform stage -> (W (d_in, d_out), mean (d_in,) or None) with y = (x - mean) @ W."""
    from ..alignment.AlignCCA import AlignCCA
    from ..alignment.pca import PCA
    from ..decomposition.NoCenterPCA import NoCenterPCA
    if isinstance(st, PCA):
        return np.asarray(st.components_, dtype=np.float64).T, np.asarray(st.mean_, dtype=np.float64)
    if isinstance(st, NoCenterPCA):
        return np.asarray(st.components_, dtype=np.float64), None
    if isinstance(st, AlignCCA):
        if st.return_space not in ('b_to_a', 'a_to_b'):
            raise ValueError("AlignCCA stage needs return_space 'b_to_a' or 'a_to_b' (one input, one output space)")
        if not st._check_fit():
            raise RuntimeError('Must call fit() before transforming data.')
        return st._map(st.return_space).cpu().numpy(), None
    if isinstance(st, (tuple, list)) and len(st) == 2:
        W = np.asarray(st[0], dtype=np.float64)
        return W, (None if st[1] is None else np.asarray(st[1], dtype=np.float64))
    raise TypeError(f'cannot fold a {type(st).__name__} into an affine feature map')


def feature_map_from(*stages):
    """Fold fitted transforms applied in order (alignment.pca.PCA, NoCenterPCA, AlignCCA 'b_to_a' / 'a_to_b', or a raw
    (W, mean)) into one (W, c) with  stages(x) = x @ W + c.  Every stage is (x - mean) @ W, so the chain is affine."""
    if not stages:
        raise ValueError('feature_map_from needs at least one stage')
    W = c = None
    for st in stages:
        Ws, m = _stage_affine(st)
        if W is None:
            W, c = Ws.copy(), np.zeros(Ws.shape[1])
        else:
            if W.shape[1] != Ws.shape[0]:
                raise ValueError(f'stage of input width {Ws.shape[0]} after a stage of output width {W.shape[1]}')
            W, c = W @ Ws, c @ Ws
        if m is not None:
            c = c - m @ Ws
    return W, c


def _per_stream(value, n_streams, is_single):
    """`value` given once (is_single(value)) or once per stream -> list of n_streams."""
    if is_single(value):
        return [value] * n_streams
    value = list(value)
    if len(value) != n_streams:
        raise ValueError(f'{len(value)} per-stream entries for {n_streams} streams')
    return value


class RealtimePipeline:
    """Raw bins (n_streams, k, n_channels, bin_samples) float64 -> logits and CTC tokens per stream.  See the module
    docstring for the launch chain; ``step`` replays one captured graph per prediction (``use_graph``).
    decoder='greedy' (default): ``decoded`` holds the greedy collapse.  decoder='beam': the prefix beam search of
    realtime_sim.decode over the log-softmax of the logits, beam_size wide, advanced one frame per prediction on the
    device; ``decoded`` / ``beam_nll`` read its best prefix (at most max_steps predictions between resets)."""

    def __init__(self, model, bandpassCoefs, n_channels, bin_samples, n_streams=1, bad_channels=None, filt_ics=None,
                 feature_map=None, use_graph=True, max_tokens=4096, decoder='greedy', beam_size=100, max_steps=4096):
        rnn = model.rnn.rnn
        if rnn.bidirectional:
            raise ValueError('the realtime pipeline needs a unidirectional model')
        dev = next(model.parameters()).device
        if dev.type != 'cuda':
            raise RuntimeError('RealtimePipeline needs the model on the GPU (no CPU fallback)')
        if not 1 <= n_streams <= 8:
            raise ValueError('1..8 streams per pipeline')
        self.win, self.stride = int(model.win_size), int(model.stride)
        if self.win < self.stride:
            raise ValueError(f'win_size {self.win} < stride {self.stride}: frames would be skipped')
        if max_tokens < 1:
            raise ValueError('max_tokens must be >= 1')
        if decoder not in ('greedy', 'beam'):
            raise ValueError(f"decoder {decoder!r}: 'greedy' or 'beam'")
        self.model, self.B, self.dev, self._call = model, int(n_streams), dev, call
        self.C, self.Tn = int(n_channels), int(bin_samples)
        self.H, self.L, self.K = rnn.hidden_size, rnn.num_layers, rnn.input_size
        self.n_classes, self.blank, self.max_tokens = model.classifier.fc.out_features, int(model.blank), int(max_tokens)
        B, C, S = self.B, self.C, 1 << (self.B - 1).bit_length()

        # ---- frontend: coefficients, good-channel masks, filter state
        b, a, zi = _split_coefs(bandpassCoefs, C, None)
        self.bands, self.taps = b.shape
        self.iir = a is not None
        self._b = torch.from_numpy(b).to(dev)
        self._a = None if a is None else torch.from_numpy(a).to(dev)
        if self.iir:
            if filt_ics is not None:
                zi = np.asarray(filt_ics, dtype=np.float64)
            want = (self.bands, C, self.taps - 1)
            if zi.shape == want:
                zi = np.broadcast_to(zi, (B,) + want)
            if zi.shape != (B,) + want:
                raise ValueError(f'filt_ics of shape {zi.shape}: expected {want} or {(B,) + want}')
            self._zi0 = torch.from_numpy(np.array(zi, dtype=np.float64, order='C')).to(dev)
            self._zi = self._zi0.clone()
        else:
            self._zi0 = self._zi = None
        single_bad = lambda v: v is None or all(e is not None and np.ndim(e) == 0 for e in v)
        bads = _per_stream(bad_channels, B, single_bad)
        self._good = torch.from_numpy(np.stack([_good_mask(C, bc) for bc in bads])).to(dev)

        # ---- feature map (W, c) per stream; all-identity runs the exact cast path (W = NULL)
        single_map = lambda v: v is None or (len(v) == 2 and not isinstance(v[0], (tuple, list)) and v[0] is not None
                                             and np.ndim(v[0]) == 2)
        maps = _per_stream(feature_map, B, single_map)
        if all(m is None for m in maps):
            self.d, self._W, self._c = C, None, None
        else:
            ds = {C if m is None else np.shape(m[0])[1] for m in maps}
            if len(ds) != 1:
                raise ValueError(f'feature maps of different widths {sorted(ds)}')
            self.d = ds.pop()
            Ws, cs = [], []
            for m in maps:
                Wm = np.eye(C) if m is None else np.asarray(m[0], dtype=np.float64)
                cm = np.zeros(self.d) if m is None or m[1] is None else np.asarray(m[1], dtype=np.float64)
                if Wm.shape != (C, self.d) or cm.shape != (self.d,):
                    raise ValueError(f'feature map W {Wm.shape}, c {cm.shape}: expected {(C, self.d)}, {(self.d,)}')
                Ws.append(Wm)
                cs.append(cm)
            self._W = torch.from_numpy(np.ascontiguousarray(np.stack(Ws))).to(dev)
            self._c = torch.from_numpy(np.ascontiguousarray(np.stack(cs))).to(dev)
        if self.win * self.d != self.K:
            raise ValueError(f'input_size {self.K} != win_size * d = {self.win} * {self.d}')

        # ---- static device buffers (rows padded to S = power of two >= B for the GEMV kernels)
        kmax = max(self.stride, self.win - self.stride, 1)
        self._bins = torch.zeros(B, self.stride, C, self.Tn, dtype=_F64, device=dev)
        self._power = torch.zeros(B, kmax, C, dtype=_F64, device=dev)
        self._ws_bytes = int(lib().xps_pipe_frontend_f64_workspace(B, C, self.Tn, self.bands))
        self._ws = workspace(self._ws_bytes, dev)
        self.wbuf = torch.zeros(2, S, self.K, dtype=torch.float32, device=dev)             # ping-pong windows
        self.hbuf = torch.zeros(2, self.L, S, self.H, dtype=torch.float32, device=dev)     # ping-pong hidden state
        self._logits = torch.zeros(S, self.n_classes, dtype=torch.float32, device=dev)
        self._token = torch.zeros(S, dtype=torch.int64, device=dev)
        self._state = torch.zeros(B, 3, dtype=torch.int32, device=dev)
        self._tokens = torch.zeros(B, self.max_tokens, dtype=torch.int64, device=dev)
        self.decoder = decoder
        if decoder == 'beam':
            check_beam_sizes(int(beam_size), self.n_classes, self.blank)
            if not 1 <= max_steps <= 1 << 20:
                raise ValueError('max_steps outside 1..2^20')
            self.beam_size, self.max_steps = int(beam_size), int(max_steps)
            self._bstate_bytes = int(lib().xps_ctc_beam_state_bytes(B, self.beam_size, self.max_steps))
            self._bstate = torch.zeros(self._bstate_bytes, dtype=torch.uint8, device=dev)
            self._bprefix = torch.zeros(self.max_steps, dtype=torch.int64, device=dev)
            self._blen = torch.zeros(1, dtype=torch.int64, device=dev)
            self._bnll = torch.zeros(1, dtype=torch.float64, device=dev)
        self._params = [tuple(p.detach().contiguous() for p in _layer_params(rnn, l, 1)[0]) for l in range(self.L)]
        self._fc = (model.classifier.fc.weight.detach().contiguous(), model.classifier.fc.bias.detach().contiguous())
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

    # ---- state ---------------------------------------------------------------------------------------------------
    @torch.no_grad()
    def reset(self):
        """Filter state, window, h = model.h0, decoded tokens and frame counter back to the start."""
        if self._zi is not None:
            self._zi.copy_(self._zi0)
        self.wbuf.zero_()
        self.hbuf.zero_()
        self.hbuf[:, :, :self.B] = self.model.h0.detach().expand(-1, self.B, -1)
        self._state.zero_()
        self._state[:, 0] = -1
        if self.decoder == 'beam':
            self._beam_headers().zero_()      # an all-zero header is the empty beam
        self._logits.zero_()
        self._token.zero_()
        self.parity, self.frames, self.n_pred, self._last_k = 0, 0, 0, 0

    @property
    def logits(self):
        return self._logits[:self.B]

    @property
    def token(self):
        return self._token[:self.B]

    @property
    def features(self):
        """The current window of every stream, (n_streams, win_size, d) float32 (device)."""
        return self.wbuf[self.parity, :self.B].view(self.B, self.win, self.d)

    @property
    def filter_state(self):
        """The carried IIR state (n_streams, bands, n_channels, order) float64 (device); None for FIR."""
        return self._zi

    @property
    def power(self):
        """Per-frame band power of the last prime / step, (n_streams, k, n_channels) float64 (device)."""
        k = self._last_k                      # the frontend writes [n_streams][k][C] packed for the k of its launch
        return self._power.view(-1)[:self.B * k * self.C].view(self.B, k, self.C)

    def _beam_headers(self):
        """The int32 header {step, n_members, overflow, 0} of every stream's beam state (include/xps.h), (n_streams, 4)."""
        return self._bstate.view(self.B, -1)[:, :16].view(torch.int32)

    def _beam_readout(self, s):
        if not 0 <= s < self.B:
            raise IndexError(f'stream {s} of {self.B}')
        if int(self._beam_headers()[s, 2]):
            raise RuntimeError(f'stream {s} ran more than max_steps = {self.max_steps} beam-search steps')
        self._call('xps_ctc_beam_readout', self._bstate.data_ptr(), self._bstate_bytes, self.B, self.beam_size,
                   self.max_steps, s, self._bprefix.data_ptr(), self._blen.data_ptr(), self._bnll.data_ptr(),
                   stream())
        return self._bprefix[:int(self._blen)].clone()

    def beam_nll(self, s):
        """-log p of stream s's best beam prefix so far (float); raises after a max_steps overflow."""
        if self.decoder != 'beam':
            raise RuntimeError("beam_nll needs decoder='beam'")
        self._beam_readout(s)
        return float(self._bnll)

    def decoded(self, s):
        """CTC tokens of stream s so far (1-D LongTensor, device): the greedy collapse, or with decoder='beam' the beam's
        best prefix; raises after a token-buffer (greedy) or max_steps (beam) overflow."""
        if self.decoder == 'beam':
            return self._beam_readout(s)
        if not 0 <= s < self.B:
            raise IndexError(f'stream {s} of {self.B}')
        _, n, over = (int(v) for v in self._state[s].cpu())
        if over:
            raise RuntimeError(f'stream {s} decoded more than max_tokens = {self.max_tokens} tokens')
        return self._tokens[s, :n].clone()

    # ---- launches --------------------------------------------------------------------------------------------------
    def _frontend(self, bins, k, st):
        self._call('xps_pipe_frontend_f64', bins.data_ptr(), self.B, k, self.C, self.Tn, self._good.data_ptr(),
                   self._b.data_ptr(), ptr(self._a), self.bands, self.taps, ptr(self._zi), self._power.data_ptr(),
                   self._ws.data_ptr(), self._ws_bytes, st)

    def _shift(self, k, src, dst, st):
        self._call('xps_window_shift_f32', self._power.data_ptr(), k, self.C, ptr(self._W), ptr(self._c),
                   src.data_ptr(), dst.data_ptr(), self.win, self.d, self.B, st)

    @torch.no_grad()
    def _body(self, par):
        st = stream()
        self._frontend(self._bins, self.stride, st)
        self._shift(self.stride, self.wbuf[par], self.wbuf[par ^ 1], st)
        src, dst = self.hbuf[par], self.hbuf[par ^ 1]
        inp, k = self.wbuf[par ^ 1], self.K
        for l, (w_ih, w_hh, b_ih, b_hh) in enumerate(self._params):
            self._call('xps_gru_cell_gemv_f32', inp.data_ptr(), k, w_ih.data_ptr(), w_hh.data_ptr(), b_ih.data_ptr(),
                       b_hh.data_ptr(), src[l].data_ptr(), dst[l].data_ptr(), self.H, self.B, st)
            inp, k = dst[l], self.H
        self._call('xps_gemv_f32', inp.data_ptr(), self._fc[0].data_ptr(), self._fc[1].data_ptr(), self._logits.data_ptr(),
                   self.n_classes, self.H, self.B, st)
        self._call('xps_ctc_collapse_f32', self._logits.data_ptr(), self.n_classes, self.blank, self._token.data_ptr(),
                   self._state.data_ptr(), self._tokens.data_ptr(), self.max_tokens, self.B, st)
        if self.decoder == 'beam':
            self._call('xps_ctc_beam_step_f32', self._logits.data_ptr(), self.n_classes, self.blank, self.beam_size,
                       self.max_steps, self._bstate.data_ptr(), self._bstate_bytes, self.B, st)

    def _check_bins(self, bins, k):
        want = (self.B, k, self.C, self.Tn)
        if tuple(bins.shape) != want:
            raise ValueError(f'bins of shape {tuple(bins.shape)}: expected {want}')

    @torch.no_grad()
    def prime(self, bins):
        """(n_streams, win_size - stride, n_channels, bin_samples) float64: the frames before the first prediction
        (frontend and window only)."""
        k = self.win - self.stride
        self._check_bins(bins, k)
        if k == 0:
            return
        bd = torch.as_tensor(bins, dtype=_F64).to(self.dev).contiguous()
        st = stream()
        self._frontend(bd, k, st)
        cur, nxt = self.wbuf[self.parity], self.wbuf[self.parity ^ 1]
        self._shift(k, cur, nxt, st)
        cur.copy_(nxt)                        # the window stays in the buffer of the current parity (h's)
        self.frames += k
        self._last_k = k

    @torch.no_grad()
    def step(self, bins=None):
        """(n_streams, stride, n_channels, bin_samples) float64 host or device (None: the static buffer as it is) ->
        logits (n_streams, n_classes) in a static buffer; ``self.token`` holds the argmax."""
        if self.frames < self.win - self.stride:
            raise RuntimeError('prime() the first win_size - stride bins before the first step')
        if bins is not None:
            self._check_bins(bins, self.stride)
            self._bins.copy_(torch.as_tensor(bins, dtype=_F64), non_blocking=True)
        if self.graphs is not None:
            self.graphs[self.parity].replay()
        else:
            self._body(self.parity)
        self.parity ^= 1
        self.frames += self.stride
        self.n_pred += 1
        self._last_k = self.stride
        return self.logits

    @torch.no_grad()
    def run(self, bins_seq):
        """(n_streams, n_bins, n_channels, bin_samples) -> (logits (n_streams, n_pred, n_classes), [decoded(s)]).
        Starts from reset(); n_pred = (n_bins - win_size) // stride + 1; trailing bins that complete no stride are not
        consumed."""
        bins_seq = torch.as_tensor(bins_seq, dtype=_F64)
        if bins_seq.dim() != 4 or (bins_seq.shape[0], bins_seq.shape[2], bins_seq.shape[3]) != (self.B, self.C, self.Tn):
            raise ValueError(f'bins_seq of shape {tuple(bins_seq.shape)}: expected ({self.B}, n_bins, {self.C}, {self.Tn})')
        n_bins = bins_seq.shape[1]
        if n_bins < self.win:
            raise ValueError(f'{n_bins} bins make no prediction (win_size {self.win})')
        n_pred = (n_bins - self.win) // self.stride + 1
        bins_seq = bins_seq.to(self.dev)
        self.reset()
        p = self.win - self.stride
        self.prime(bins_seq[:, :p])
        out = torch.empty(self.B, n_pred, self.n_classes, dtype=torch.float32, device=self.dev)
        for w in range(n_pred):
            out[:, w] = self.step(bins_seq[:, p + w * self.stride:p + (w + 1) * self.stride])
        return out, [self.decoded(s) for s in range(self.B)]
