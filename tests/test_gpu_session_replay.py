"""Session replay (realtime_sim/session_replay.py, xps_hg_trials_f64): the frontend over N recorded trials in one launch,
bit for bit the streaming frontend (xps_pipe_frontend_f64) and RealtimePipeline's window frames; the batched model path
against RealtimePipeline.run, the beam search, the PER and the CPU oracles.  Seeded synthetic data throughout."""
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from weights import weights_from_seed  # noqa: E402


def _rt():
    from cross_patient_speech_decoding_amd import realtime_sim
    from cross_patient_speech_decoding_amd.realtime_sim import realtime_processing as rp
    return realtime_sim, rp


def _iir(nb, order):
    import scipy.signal as signal
    out = []
    for k in range(nb):
        b, a = signal.butter(order, [60 + 12 * k, 72 + 12 * k], btype='band', fs=2000)
        out.append(np.stack([a, b], axis=1))
    return np.stack(out)


def _fir(nb, taps):
    import scipy.signal as signal
    return np.stack([signal.firwin(taps, [60 + 12 * k, 72 + 12 * k], pass_zero=False, fs=2000) for k in range(nb)])


def _model_cpu(C_in, win, stride, H=16, L=1, ncls=7, seed=11):
    from cross_patient_speech_decoding_amd.realtime_sim import RealtimeRNNModel
    m = RealtimeRNNModel(win * C_in, H, L, ncls, dropout=0.0, win_size=win, stride=stride)
    sd = weights_from_seed(m.state_dict(), seed)
    sd['h0'] = torch.from_numpy(np.random.default_rng(seed + 1).uniform(-0.5, 0.5, (L, 1, H)).astype(np.float32))
    m.load_state_dict(sd)
    return m.eval()


def _model(*args, **kw):
    return _model_cpu(*args, **kw).cuda()


def _streaming(raw, b, a, good, zi0):
    """The parent's bulk path: xps_pipe_frontend_f64 with k = n_bins over groups of up to 8 trials as streams.
    raw (N, n_bins, C, Tn) float64 device, good (N, C) uint8 device, zi0 (N, bands, C, taps-1) device or None (FIR)
    -> power (N, n_bins, C), state (N, ...) or None."""
    from cross_patient_speech_decoding_amd._lib import call, lib
    N, n_bins, C, Tn = raw.shape
    bands, taps = b.shape
    power = torch.empty(N, n_bins, C, dtype=torch.float64, device=raw.device)
    state = None if zi0 is None else zi0.clone()
    st = torch.cuda.current_stream().cuda_stream
    for s0 in range(0, N, 8):
        n = min(8, N - s0)
        nbytes = int(lib().xps_pipe_frontend_f64_workspace(n, C, Tn, bands))
        ws = torch.empty(nbytes, dtype=torch.uint8, device=raw.device)
        call('xps_pipe_frontend_f64', raw[s0:s0 + n].data_ptr(), n, n_bins, C, Tn, good[s0:s0 + n].data_ptr(), b.data_ptr(),
             None if a is None else a.data_ptr(), bands, taps, None if state is None else state[s0:s0 + n].data_ptr(),
             power[s0:s0 + n].data_ptr(), ws.data_ptr(), nbytes, st)
    return power, state


# (iir, C, bands, taps, Tn, N, bad channels, per-trial zi0, float32 input); every value of the issue's grid occurs, the
# bands == 8 path and a general band count both meet C = 130, and (5, 2048) is a bin too large to stage in LDS (both paths)
GRID = [
    (True, 128, 8, 9, 40, 9, True, False, False),
    (True, 130, 8, 9, 40, 300, True, True, False),
    (True, 130, 3, 9, 40, 9, False, False, True),
    (True, 64, 8, 3, 7, 1, False, True, True),
    (True, 5, 1, 17, 7, 9, True, False, False),
    (True, 64, 8, 17, 40, 9, True, True, False),
    (True, 5, 3, 3, 40, 300, False, True, False),
    (False, 128, 8, 9, 40, 9, True, False, False),
    (False, 130, 3, 17, 7, 9, False, False, True),
    (False, 64, 1, 3, 40, 1, True, False, False),
    (True, 5, 8, 9, 2048, 3, True, False, False),
    (False, 6, 8, 29, 40, 9, False, False, False),
    (True, 5, 3, 9, 2048, 3, True, False, False),         # general path, bin not staged
    (False, 6, 3, 29, 40, 9, False, False, True),         # general path, more than 17 taps
    (True, 64, 8, 9, 37, 9, True, True, False),           # odd Tn > 16: uneven leaves (18 -> 9 + 9, 19 -> 9 + 10)
    (True, 20, 8, 5, 301, 3, False, False, False),        # 301 = 150 + 151 -> ... : a deeper, uneven tree
]


@pytest.mark.parametrize('iir,C,bands,taps,Tn,N,bad,zi_per_trial,f32', GRID)
def test_bitwise_against_the_streaming_frontend(iir, C, bands, taps, Tn, N, bad, zi_per_trial, f32):
    rt, rp = _rt()
    n_bins = 5
    rng = np.random.default_rng(1000 * C + 10 * bands + taps + N)
    coefs = _iir(bands, (taps - 1) // 2) if iir else _fir(bands, taps)
    b, a, zi = rp._split_coefs(coefs, C, None)
    assert b.shape == (bands, taps)
    raw = rng.standard_normal((N, n_bins, C, Tn)) * 30.0
    if f32:
        raw = raw.astype(np.float32)
    bads = sorted(rng.choice(C, 2, replace=False).tolist()) if bad else None
    ics = None
    if iir:
        ics = zi * rng.uniform(0.5, 1.5, (N,) + zi.shape) if zi_per_trial else zi
    dev = torch.device('cuda')
    raw_d = torch.from_numpy(raw).to(dev)
    good = torch.from_numpy(np.tile(rp._good_mask(C, bads), (N, 1))).to(dev)
    zi_full = None if not iir else torch.from_numpy(np.array(np.broadcast_to(ics, (N,) + zi.shape), order='C')).to(dev)
    ref_p, ref_z = _streaming(raw_d.double(), torch.from_numpy(b).to(dev), None if a is None else torch.from_numpy(a).to(dev),
                              good, zi_full)
    got_p, got_z = rt.process_HG_trials(raw_d, coefs, bad_channels=bads, filt_ics=ics, return_state=True)
    assert got_p.dtype == torch.float64 and got_p.shape == (N, n_bins, C)
    assert torch.isfinite(ref_p).all()
    assert torch.equal(got_p, ref_p)
    if iir:
        assert torch.equal(got_z, ref_z)
    else:
        assert got_z is None
    if f32:                                   # widened on load: the same values as float64 give the same bits
        assert torch.equal(rt.process_HG_trials(raw_d.double(), coefs, bad_channels=bads, filt_ics=ics), got_p)


def test_against_the_cpu_oracle_and_the_golden_bins(golden_dir):
    """One trial looped bin by bin through the CPU oracle: the IIR chain bit for bit, the FIR path to the rtol 1e-13
    tests/test_gpu_processing.py allows process_HG; the golden bins as a one-trial session."""
    from oracle import realtime_processing_oracle as po
    rt, rp = _rt()
    rng = np.random.default_rng(5)
    for C, Tn, nb, order in ((128, 40, 8, 3), (37, 301, 5, 4), (9, 7, 1, 1)):
        coefs = _iir(nb, order)
        trial = rng.standard_normal((1, 4, C, Tn))
        ics, rows = None, []
        for j in range(4):
            p, ics = po.process_hg(trial[0, j], coefs, bad_channels=[1], filt_ics=ics)
            rows.append(p)
        got, state = rt.process_HG_trials(trial, coefs, bad_channels=[1], return_state=True)
        np.testing.assert_array_equal(got.cpu().numpy()[0], np.stack(rows))
        np.testing.assert_array_equal(state.cpu().numpy()[0], ics)
    g = np.load(os.path.join(golden_dir, 'realtime_processing.npz'))
    bad = [int(v) for v in g['bad']]
    got, state = rt.process_HG_trials(g['bins'][None], g['iir'], bad_channels=bad, return_state=True)
    for i in range(3):
        np.testing.assert_array_equal(got.cpu().numpy()[0, i], g[f'iir_power{i}'])
    np.testing.assert_array_equal(state.cpu().numpy()[0], g['iir_ics2'])
    pf = rt.process_HG_trials(g['bins'][None], g['fir'])
    np.testing.assert_allclose(pf.cpu().numpy()[0, 1], g['fir_power1'], rtol=1e-13)
    for i in range(3):
        ref, _ = po.process_hg(g['bins'][i], g['fir'])
        np.testing.assert_allclose(pf.cpu().numpy()[0, i], ref, rtol=1e-13)


@pytest.mark.parametrize('bands', [8, 3])
def test_padded_trials(bands):
    rt, rp = _rt()
    C, Tn, N, n_bins = 20, 40, 6, 7
    coefs = _iir(bands, 4)
    rng = np.random.default_rng(77 + bands)
    raw = torch.from_numpy(rng.standard_normal((N, n_bins, C, Tn))).cuda()
    lengths = [7, 3, 0, 1, 6, 7]
    p, z = rt.process_HG_trials(raw, coefs, bad_channels=[4], lengths=lengths, return_state=True)
    zi0 = torch.from_numpy(rp._split_coefs(coefs, C, None)[2]).cuda()
    for n, L in enumerate(lengths):
        assert torch.count_nonzero(p[n, L:]) == 0
        if L == 0:
            assert torch.equal(z[n], zi0)
            continue
        alone, za = rt.process_HG_trials(raw[n:n + 1, :L], coefs, bad_channels=[4], return_state=True)
        assert torch.equal(p[n, :L], alone[0])
        assert torch.equal(z[n], za[0])
    with pytest.raises(ValueError):
        rt.process_HG_trials(raw, coefs, lengths=[8] * N)


def test_independence_of_the_batch():
    rt, rp = _rt()
    C, Tn, N, n_bins, d = 128, 40, 300, 4, 30
    coefs = _iir(8, 4)
    rng = np.random.default_rng(31)
    raw = torch.from_numpy(rng.standard_normal((N, n_bins, C, Tn)).astype(np.float32)).cuda()
    maps = [(rng.standard_normal((C, d)), rng.standard_normal(d)) for _ in range(2)]
    sr = rt.SessionReplay(_model(d, 3, 1), coefs, C, Tn, bad_channels=[[1], [2, 3]], feature_map=maps)
    patient = np.arange(N) % 2
    full = sr.features(raw, patient=patient)
    assert full.dtype == torch.float32 and full.shape == (N, n_bins, d)
    assert torch.equal(sr.features(raw, patient=patient), full)
    for i in (0, 137, 299):
        assert torch.equal(sr.features(raw[i:i + 1], patient=int(patient[i]))[0], full[i])


def _pca_cca(C, d, seed=0):
    from cross_patient_speech_decoding_amd.alignment import AlignCCA
    from cross_patient_speech_decoding_amd.alignment.pca import PCA
    from cross_patient_speech_decoding_amd.utils.synthetic import make_patient
    Xb_raw, yb = make_patient(1 + seed, 256, T=20, C=C)
    Xb_raw = np.abs(Xb_raw.astype(np.float64)) * 0.1
    pca = PCA(n_components=d).fit(Xb_raw.reshape(-1, C))
    Xb = pca.transform(Xb_raw)
    Xa, ya = make_patient(0, 256, T=20, C=d)
    cca = AlignCCA(return_space='b_to_a')
    cca.fit(Xa, Xb, ya, yb)
    return pca, cca


@pytest.mark.parametrize('mapped', [False, True])
def test_feature_parity_with_the_pipeline(mapped):
    """SessionReplay.features against the frames RealtimePipeline holds in its window, at every prediction."""
    rt, rp = _rt()
    C, Tn, win, stride, n_bins, B = 128, 40, 6, 4, 18, 3
    d = 30 if mapped else C
    coefs = _iir(8, 4)
    maps = [rt.feature_map_from(*_pca_cca(C, d, seed=s)) for s in range(B)] if mapped else None
    bads = [[1, 5], [0], [C - 1, 2, 3]]
    m = _model(d, win, stride)
    pipe = rt.RealtimePipeline(m, coefs, C, Tn, n_streams=B, bad_channels=bads, feature_map=maps)
    sr = rt.SessionReplay(m, coefs, C, Tn, bad_channels=bads, feature_map=maps)
    rng = np.random.default_rng(9 + mapped)
    bins = rng.standard_normal((B, n_bins, C, Tn)) * 20.0
    feats = sr.features(bins, patient=np.arange(B))
    pipe.prime(bins[:, :win - stride])
    n_pred = (n_bins - win) // stride + 1
    for w in range(n_pred):
        j0 = win - stride + w * stride
        pipe.step(bins[:, j0:j0 + stride])
        assert torch.equal(pipe.features, feats[:, j0 + stride - win:j0 + stride])
    assert n_pred == 4


C5 = dict(C=128, Tn=40, win=14, stride=4, H=128, L=2, ncls=11, n_bins=50, N=16, seed=505, data_seed=611)


def _config5_data():
    rng = np.random.default_rng(C5['data_seed'])
    return rng.standard_normal((C5['N'], C5['n_bins'], C5['C'], C5['Tn'])) * 50.0


def _oracle_logits(m, bins, coefs, bads):
    from oracle import realtime_processing_oracle as po
    from oracle.realtime_oracle import RealtimeOracle
    feats = []
    for s in range(bins.shape[0]):
        ics, rows = None, []
        for j in range(bins.shape[1]):
            p, ics = po.process_hg(bins[s, j], coefs, bad_channels=bads, filt_ics=ics)
            rows.append(p)
        feats.append(np.stack(rows).astype(np.float32))
    orc = RealtimeOracle(C5['win'] * C5['C'], C5['H'], C5['L'], C5['ncls'], C5['win'], C5['stride'])
    orc.load_reference_state({k: v.detach().cpu() for k, v in m.state_dict().items()})
    orc.eval()
    with torch.no_grad():
        return orc(torch.from_numpy(np.stack(feats)))


def test_end_to_end_config5_against_the_pipeline():
    """16 trials at the config-5 shape: SessionReplay.run against RealtimePipeline.run 8 trials at a time (logits 1e-4,
    the bound tests/test_gpu_realtime.py has between graph replay and full forward; identical greedy tokens), the beam
    search against beam_decode_batch on the replay's own logits, the PER against calc_PER.  The oracle's top-2 logit
    margin on these inputs is asserted to be >= 1e-3 at every frame, so no token hangs on a near tie."""
    rt, rp = _rt()
    torch.set_num_threads(min(8, len(os.sched_getaffinity(0))))
    C, Tn, N = C5['C'], C5['Tn'], C5['N']
    m = _model(C, C5['win'], C5['stride'], H=C5['H'], L=C5['L'], ncls=C5['ncls'], seed=C5['seed'])
    coefs = _iir(8, 4)
    bads = [5, 77]
    bins = _config5_data()
    ref = _oracle_logits(m, bins, coefs, bads)
    top2 = ref.topk(2, dim=-1).values
    margin = (top2[..., 0] - top2[..., 1]).min().item()
    print('oracle top-2 margin', margin)
    assert margin >= 1e-3
    sr = rt.SessionReplay(m, coefs, C, Tn, bad_channels=bads)
    res = sr.run(bins)
    n_pred = (C5['n_bins'] - C5['win']) // C5['stride'] + 1
    assert res.logits.shape == (N, n_pred, C5['ncls'])
    pipe = rt.RealtimePipeline(m, coefs, C, Tn, n_streams=8, bad_channels=[bads] * 8)
    dec = res.decoded()
    for s0 in range(0, N, 8):
        logits, toks = pipe.run(bins[s0:s0 + 8])
        err = (logits - res.logits[s0:s0 + 8]).abs().max().item()
        print('trials', s0, 'logit err', err)
        assert err <= 1e-4
        for s in range(8):
            assert torch.equal(toks[s], dec[s0 + s])
    assert (res.logits.cpu() - ref).abs().max().item() <= 1e-4
    assert torch.equal(res.logits.argmax(-1).cpu(), ref.argmax(-1))
    # beam: ragged trials, the replay's own logits with the trial lengths
    lengths = np.array([50, 14, 17, 18, 33, 50, 49, 21] * 2)
    srb = rt.SessionReplay(m, coefs, C, Tn, bad_channels=bads, decoder='beam', beam_size=16)
    rb = srb.run(bins, lengths=lengths)
    pred = (lengths - C5['win']) // C5['stride'] + 1
    assert rb.pred_lengths.cpu().tolist() == pred.tolist()
    want, nll = rt.beam_decode_batch(rb.logits, input_lengths=pred, beam_size=16, blank=0, from_logits=True, return_nll=True)
    got = rb.decoded()
    for i in range(N):
        assert torch.equal(got[i], want[i])
    assert torch.equal(rb.beam_nll, nll)
    # greedy with lengths: each trial's tokens are those of its own valid predictions
    rg = sr.run(bins, lengths=lengths)
    for i, toks in enumerate(rg.decoded()):
        assert torch.equal(toks, rt.greedy_decode_batch(rg.logits[i:i + 1, :pred[i]], blank=0)[0])
        assert torch.equal(rg.logits[i, :pred[i]], res.logits[i, :pred[i]])
    with pytest.raises(ValueError, match='13 bins'):
        sr.run(bins, lengths=[13] + [50] * (N - 1))


def test_per_against_calc_per():
    rt, rp = _rt()
    C, Tn, win, stride, N, n_bins = 16, 40, 4, 2, 12, 40
    m = _model(C, win, stride, H=16, L=1, ncls=7, seed=3)
    with torch.no_grad():                     # no blank bias: the greedy path emits tokens
        m.classifier.fc.bias.zero_()
    rng = np.random.default_rng(12)
    bins = rng.standard_normal((N, n_bins, C, Tn)) * 40.0
    targets = rng.integers(1, 7, (N, 5))
    tl = rng.integers(1, 6, N)
    sr = rt.SessionReplay(m, _iir(4, 2), C, Tn)
    res = sr.run(bins, targets=targets, target_lengths=tl)
    assert res.per.dim() == 0 and res.per.is_cuda
    assert int(res.token_lengths.sum()) > 0
    want = rt.calc_PER(rt.greedy_decode_batch(res.logits, blank=0), torch.from_numpy(targets), torch.from_numpy(tl))
    assert float(res.per) == want


def test_device_patient_index_out_of_range_gives_nan_rows():
    """A device-resident patient index is not read back; the kernel checks it, under the identity map too."""
    rt, rp = _rt()
    C, Tn = 8, 40
    sr = rt.SessionReplay(_model(C, 3, 1), _iir(2, 2), C, Tn, bad_channels=[[1], [2]])
    raw = torch.from_numpy(np.random.default_rng(1).standard_normal((3, 4, C, Tn))).cuda()
    f = sr.features(raw, patient=torch.tensor([0, 1, 5], device='cuda'))
    assert torch.isfinite(f[:2]).all() and torch.isnan(f[2]).all()
    with pytest.raises(ValueError, match='outside'):
        sr.features(raw, patient=[0, 1, 5])
