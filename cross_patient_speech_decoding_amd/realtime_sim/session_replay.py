"""Batched session replay on the MI355X: every raw ECoG trial of a recorded session -> high-gamma power -> alignment map ->
features -> GRU -> CTC tokens (and PER), in a handful of launches for the whole session.

RealtimePipeline makes one prediction per graph replay for up to 8 streams; SessionReplay runs the same arithmetic in
bulk.  The frontend is one launch (xps_hg_trials_f64: CAR -> band-pass with carried state -> RMS -> float32(power @ W + c)
for all trials); its features are bit for bit the frames the streaming pipeline puts in its window, so a model trained on
``features`` of recorded sessions sees at serving time what it was trained on.  The model part is the batched training
path (RealtimeRNNModel.forward_tm, greedy_decode_device / the batched prefix beam search, per_device).

Trials of several patients share a launch: each patient has its own bad channels, alignment map (feature_map_from) and
start state, and ``patient`` says which trial is whose.  There is no CPU fallback."""
import numpy as np
import torch

from .ctc_align import forced_align
from .ctc_occupancy import posterior_align
from .ctc_decoder import _beam_device, check_beam_sizes, greedy_decode_device
from .ctc_errors import edit_align
from .realtime_nn_model import per_device
from .realtime_processing import _check_trials, _good_mask, _hg_trials, _split_coefs, _trial_lengths, _trials_on_device

_F64 = torch.float64


class SessionResult:
    """What SessionReplay.run returns (device tensors): logits (N, n_pred, n_classes) float32; tokens (N, n_pred) int64,
    the decoded labels of each trial, then -1; token_lengths (N,) int64; pred_lengths (N,) int64, the valid predictions
    of each trial; features (N, n_bins, d) float32; beam_nll (N,) float64 with decoder='beam', else None; per, a 0-dim
    float64 tensor, when targets were given, else None; blank, the model's blank label (align needs it)."""

    def __init__(self, logits, tokens, token_lengths, pred_lengths, features, beam_nll=None, per=None, blank=0):
        self.logits, self.tokens, self.token_lengths, self.pred_lengths = logits, tokens, token_lengths, pred_lengths
        self.features, self.beam_nll, self.per = features, beam_nll, per
        self.blank = blank

    def align(self, targets, target_lengths=None):
        """Forced alignment (realtime_sim/ctc_align.py) of each trial's known targets through the log-softmax of its logits,
        over the trial's pred_lengths valid predictions -> CTCAlignment; frame w is prediction w."""
        return forced_align(torch.log_softmax(self.logits, dim=2), targets, input_lengths=self.pred_lengths,
                            target_lengths=target_lengths, blank=self.blank)

    def posterior_align(self, targets, target_lengths=None):
        """Posterior occupancies (realtime_sim/ctc_occupancy.py) of each trial's known targets through the log-softmax of its
        logits, over the trial's pred_lengths valid predictions -> CTCOccupancy; frame w is prediction w."""
        return posterior_align(torch.log_softmax(self.logits, dim=2), targets, input_lengths=self.pred_lengths,
                               target_lengths=target_lengths, blank=self.blank)

    def errors(self, targets, target_lengths=None, n_classes=None):
        """Edit-operation alignment (realtime_sim/ctc_errors.py) of each trial's decoded tokens against its known targets ->
        EditAlignment: the hits, substitutions, deletions and insertions behind `per`, the maps between the two sequences
        and, with n_classes, the phoneme confusion matrix.  The tokens are -1 padded; token_lengths govern.
        target_lengths None: all of targets' columns."""
        return edit_align(self.tokens, self.token_lengths, targets, target_lengths, n_classes=n_classes)

    def decoded(self):
        """The tokens as a list of 1-D LongTensors (one transfer of the N lengths)."""
        return [self.tokens[i, :n] for i, n in enumerate(self.token_lengths.tolist())]


def _is_single_bad(v):
    return v is None or all(e is not None and np.ndim(e) == 0 for e in v)


def _is_single_map(v):
    return v is None or (len(v) == 2 and not isinstance(v[0], (tuple, list)) and v[0] is not None and np.ndim(v[0]) == 2)


class SessionReplay:
    """Raw trials (N, n_bins, n_channels, bin_samples), float32 or float64, host or device -> features, logits, tokens.
    Arguments as RealtimePipeline's; ``bad_channels``, ``feature_map`` and ``filt_ics`` are given once or once per
    patient (filt_ics: (bands, n_channels, order) or (n_patients, bands, n_channels, order))."""

    def __init__(self, model, bandpassCoefs, n_channels, bin_samples, bad_channels=None, filt_ics=None, feature_map=None,
                 decoder='greedy', beam_size=100):
        rnn = model.rnn.rnn
        if rnn.bidirectional:
            raise ValueError('session replay needs a unidirectional model')
        if decoder not in ('greedy', 'beam'):
            raise ValueError(f"decoder {decoder!r}: 'greedy' or 'beam'")
        self.model, self.decoder, self.beam_size = model, decoder, int(beam_size)
        self.win, self.stride = int(model.win_size), int(model.stride)
        self.C, self.Tn = int(n_channels), int(bin_samples)
        self.n_classes, self.blank = model.classifier.fc.out_features, int(model.blank)
        if decoder == 'beam':
            check_beam_sizes(self.beam_size, self.n_classes, self.blank)
        C = self.C

        # ---- host side: coefficients, per-patient masks, maps and start states (all shapes checked before the device)
        b, a, zi = _split_coefs(bandpassCoefs, C, None)
        self.bands, self.taps = b.shape
        self.iir = a is not None
        bads = [bad_channels] if _is_single_bad(bad_channels) else list(bad_channels)
        maps = [feature_map] if _is_single_map(feature_map) else list(feature_map)
        if self.iir:
            if filt_ics is not None:
                zi = np.asarray(filt_ics, dtype=np.float64)
            want = (self.bands, C, self.taps - 1)
            if zi.shape != want and zi.shape[1:] != want:
                raise ValueError(f'filt_ics of shape {zi.shape}: expected {want} or (n_patients,) + {want}')
        else:
            zi = None
        counts = {len(v) for v in (bads, maps) if len(v) > 1}
        if zi is not None and zi.ndim == 4 and zi.shape[0] > 1:
            counts.add(zi.shape[0])
        if len(counts) > 1:
            raise ValueError(f'per-patient arguments for different numbers of patients: {sorted(counts)}')
        self.n_patients = P = counts.pop() if counts else 1
        bads, maps = bads * (P // len(bads)), maps * (P // len(maps))
        good = np.stack([_good_mask(C, bc) for bc in bads])
        if all(m is None for m in maps):
            self.d, W, c = C, None, None
        else:
            for m in maps:
                if m is not None and (np.ndim(m[0]) != 2 or np.shape(m[0])[0] != C):
                    raise ValueError(f'feature map W of shape {np.shape(m[0])}: expected ({C}, d)')
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
            W, c = np.ascontiguousarray(np.stack(Ws)), np.ascontiguousarray(np.stack(cs))
        if self.win * self.d != rnn.input_size:
            raise ValueError(f'input_size {rnn.input_size} != win_size * d = {self.win} * {self.d}')

        # ---- device side
        dev = next(model.parameters()).device
        if dev.type != 'cuda':
            raise RuntimeError('SessionReplay needs the model on the GPU (no CPU fallback)')
        self.dev = dev
        up = lambda x: None if x is None else torch.from_numpy(np.ascontiguousarray(x)).to(dev)
        self._b, self._a, self._zi, self._good, self._W, self._c = up(b), up(a), up(zi), up(good), up(W), up(c)

    # ---- arguments ------------------------------------------------------------------------------------------------
    def _patients(self, patient, N):
        """None / int / (N,) -> (N,) int64 device index, or None when there is one patient."""
        P = self.n_patients
        if patient is None or np.ndim(patient) == 0 and not torch.is_tensor(patient):
            p = 0 if patient is None else int(patient)
            if not 0 <= p < P:
                raise ValueError(f'patient {p} of {P}')
            return None if P == 1 else torch.full((N,), p, dtype=torch.int64, device=self.dev)
        idx = torch.as_tensor(patient)
        if tuple(idx.shape) != (N,):
            raise ValueError(f'patient of shape {tuple(idx.shape)}: expected an int or ({N},)')
        if not idx.is_cuda and N and (int(idx.min()) < 0 or int(idx.max()) >= P):
            raise ValueError(f'patient indices outside 0..{P - 1}')
        return None if P == 1 else idx.to(self.dev, torch.int64)

    def _frontend(self, raw, lengths, patient, want_power=False, lens=None):
        raw = _trials_on_device(raw, self.C, self.Tn).to(self.dev)
        N, n_bins = raw.shape[0], raw.shape[1]
        if lens is None:
            lens = _trial_lengths(lengths, N, n_bins)
        idx = self._patients(patient, N)
        good, zi, mot = self._good[0], self._zi, None
        if idx is not None:
            sel = idx.clamp(0, self.n_patients - 1)     # an index out of range gives NaN features, not a stray read
            good = self._good.index_select(0, sel)
            mot = idx.to(torch.int32)
        if zi is not None and zi.dim() == 4:
            zi = zi[0] if zi.shape[0] == 1 else zi.index_select(0, sel)
        power, _, feats = _hg_trials(raw, self._b, self._a, self.bands, self.taps, None if lens is None else lens.to(self.dev),
                                     good, zi, want_power=want_power, fmap=(self._W, self._c, self.d),
                                     map_of_trial=mot, n_maps=self.n_patients)
        return power, feats, lens

    # ---- the two entry points ---------------------------------------------------------------------------------------
    @torch.no_grad()
    def features(self, raw, lengths=None, patient=None):
        """(N, n_bins, d) float32 on the device: what the CTCHeldOut*DataModules and RealtimeRNNModel.forward take.
        ``lengths`` (N,) host integers: the bins of each trial (rows after them are zeros); ``patient``: an int or an (N,)
        index into the per-patient masks, maps and start states.  A host index is range-checked here; a device index is
        not read back: a trial whose index is out of range gets NaN features (any map, the identity included)."""
        return self._frontend(raw, lengths, patient)[1]

    @torch.no_grad()
    def run(self, raw, lengths=None, patient=None, targets=None, target_lengths=None):
        """The whole session -> SessionResult.  n_pred = (n_bins - win_size) // stride + 1, and a trial of ``lengths[n]``
        bins has (lengths[n] - win_size) // stride + 1 valid predictions, as RealtimePipeline.run; frames after them do not
        reach the decode.  ``targets`` (N, L) with ``target_lengths`` (N,) add the phoneme error rate.  ``lengths`` are
        host integers (a device tensor is copied to the host first, which waits for it); with host ``lengths``, ``patient``
        and ``target_lengths`` nothing here waits for the device."""
        raw = _check_trials(raw, self.C, self.Tn)
        lens = _trial_lengths(lengths, raw.shape[0], raw.shape[1])
        short = raw.shape[1] if lens is None else int(lens.min())
        if short < self.win:
            raise ValueError(f'{short} bins make no prediction (win_size {self.win})')
        _, feats, _ = self._frontend(raw, None, patient, lens=lens)
        N = feats.shape[0]
        was_training = self.model.training
        self.model.eval()
        try:
            logits = self.model.forward(feats)                      # (N, n_pred, n_classes)
        finally:
            self.model.train(was_training)
        n_pred = logits.shape[1]
        if lens is None:
            pred_host = None
            pred_lengths = torch.full((N,), n_pred, dtype=torch.int64, device=self.dev)
        else:
            pred_host = (lens - self.win) // self.stride + 1
            pred_lengths = pred_host.to(self.dev)
        beam_nll = None
        if self.decoder == 'beam':
            tokens, token_lengths, beam_nll = _beam_device(logits, pred_host, self.beam_size, self.blank, True)
        else:
            scores = logits
            if pred_host is not None:       # a frame after the trial's last prediction decodes as blank: it emits nothing
                pad = torch.full((self.n_classes,), -float('inf'), dtype=logits.dtype, device=self.dev)
                pad[self.blank] = 0.0
                valid = torch.arange(n_pred, device=self.dev)[None, :] < pred_lengths[:, None]
                scores = torch.where(valid[:, :, None], logits, pad)
            tokens, token_lengths = greedy_decode_device(scores, blank=self.blank)
        per = None
        if targets is not None:
            if target_lengths is None:
                raise ValueError('targets need target_lengths')
            per = per_device(tokens, token_lengths, torch.as_tensor(targets).to(self.dev), target_lengths)
        return SessionResult(logits, tokens, token_lengths, pred_lengths, feats, beam_nll, per, self.blank)
