"""Realtime pipeline (realtime_sim/realtime_pipeline.py): raw bins -> frontend -> feature map -> window -> hipGraph GRU step
-> greedy CTC tokens, against process_HG bin by bin (bit-exact powers and filter state), the host transforms, the
full-sequence model forward and the CPU oracles."""
import os
import time

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


def _model(C_in, win, stride, H=16, L=1, ncls=7, seed=11):
    from cross_patient_speech_decoding_amd.realtime_sim import RealtimeRNNModel
    m = RealtimeRNNModel(win * C_in, H, L, ncls, dropout=0.0, win_size=win, stride=stride)
    sd = weights_from_seed(m.state_dict(), seed)
    sd['h0'] = torch.from_numpy(np.random.default_rng(seed + 1).uniform(-0.5, 0.5, (L, 1, H)).astype(np.float32))
    m.load_state_dict(sd)
    return m.cuda().eval()


def _offline_power(rp, bins, coefs, bads):
    """process_HG bin by bin with carried filt_ics, per stream -> (n_streams, n_bins, C), final ics per stream."""
    pw, ics_out = [], []
    for s in range(bins.shape[0]):
        ics, rows = None, []
        for j in range(bins.shape[1]):
            p, ics = rp.process_HG(bins[s, j], coefs, bad_channels=bads[s], filt_ics=ics)
            rows.append(p)
        pw.append(np.stack(rows))
        ics_out.append(ics)
    return np.stack(pw), ics_out


@pytest.mark.parametrize('C,Tn,nb,order', [(128, 40, 8, 4), (37, 301, 5, 3)])
@pytest.mark.parametrize('n_streams', [1, 3])
def test_frontend_bit_exact_vs_process_hg(C, Tn, nb, order, n_streams):
    rt, rp = _rt()
    coefs = _iir(nb, order)
    win, stride = 6, 4
    bads = [[1, 5], [0], [C - 1, 2, 3]][:n_streams]
    pipe = rt.RealtimePipeline(_model(C, win, stride), coefs, C, Tn, n_streams=n_streams, bad_channels=bads)
    rng = np.random.default_rng(C + n_streams)
    n_bins = 14
    bins = rng.standard_normal((n_streams, n_bins, C, Tn))
    ref, ics = _offline_power(rp, bins, coefs, bads)
    got = []
    pipe.prime(bins[:, :win - stride])
    got.append(pipe.power.cpu().numpy())
    for w in range((n_bins - win) // stride + 1):
        j0 = win - stride + w * stride
        pipe.step(bins[:, j0:j0 + stride])
        got.append(pipe.power.cpu().numpy())
        # identity map: the window is float32 of the last win powers, exactly
        np.testing.assert_array_equal(pipe.features.cpu().numpy(), ref[:, j0 + stride - win:j0 + stride].astype(np.float32))
    got = np.concatenate(got, axis=1)
    np.testing.assert_array_equal(got, ref)
    zs = pipe.filter_state.cpu().numpy()
    for s in range(n_streams):
        np.testing.assert_array_equal(zs[s], ics[s])


def test_frontend_golden_bins_and_fir(golden_dir):
    rt, rp = _rt()
    g = np.load(os.path.join(golden_dir, 'realtime_processing.npz'))
    bad = [int(v) for v in g['bad']]
    C, Tn = g['bins'].shape[1:]
    pipe = rt.RealtimePipeline(_model(C, 3, 3), g['iir'], C, Tn, bad_channels=bad)
    pipe.prime(np.zeros((1, 0, C, Tn)))
    pipe.step(g['bins'][None])
    p = pipe.power.cpu().numpy()[0]
    for i in range(3):
        np.testing.assert_array_equal(p[i], g[f'iir_power{i}'])
    np.testing.assert_array_equal(pipe.filter_state.cpu().numpy()[0], g['iir_ics2'])
    # FIR: zero state in every bin, as the reference
    assert pipe.iir
    pf = rt.RealtimePipeline(_model(C, 3, 3), g['fir'], C, Tn, n_streams=2, bad_channels=[bad, []])
    assert pf.filter_state is None
    bins = np.stack([g['bins'], g['bins'][::-1]])
    pf.step(bins)
    got = pf.power.cpu().numpy()
    for s, bs in enumerate((bad, [])):
        for i in range(3):
            ref, _ = rp.process_HG(bins[s, i], g['fir'], bad_channels=bs)
            np.testing.assert_allclose(got[s, i], ref, rtol=1e-13, atol=0)


def _pca_cca(C, d, seed=0):
    from cross_patient_speech_decoding_amd.alignment import AlignCCA
    from cross_patient_speech_decoding_amd.alignment.pca import PCA
    from cross_patient_speech_decoding_amd.utils.synthetic import make_patient
    Xb_raw, yb = make_patient(1 + seed, 256, T=20, C=C)
    Xb_raw = np.abs(Xb_raw.astype(np.float64)) * 0.1            # power-like: positive, of the scale of the band power
    pca = PCA(n_components=d).fit(Xb_raw.reshape(-1, C))
    Xb = pca.transform(Xb_raw)
    Xa, ya = make_patient(0, 256, T=20, C=d)
    cca = AlignCCA(return_space='b_to_a')
    cca.fit(Xa, Xb, ya, yb)
    return pca, cca


def test_feature_map_pca_cca():
    rt, rp = _rt()
    C, Tn, d, win, stride = 128, 40, 30, 5, 4
    pca, cca = _pca_cca(C, d)
    W, c = rt.feature_map_from(pca, cca)
    assert W.shape == (C, d) and c.shape == (d,)
    rng = np.random.default_rng(3)
    X = np.abs(rng.standard_normal((50, C))) * 0.1
    two = cca.transform(pca.transform(X))
    np.testing.assert_allclose(X @ W + c, two, rtol=0, atol=1e-10 * np.abs(two).max())
    coefs = _iir(8, 4)
    pipe = rt.RealtimePipeline(_model(d, win, stride), coefs, C, Tn, feature_map=(W, c), bad_channels=[7])
    bins = rng.standard_normal((1, win - stride + 2 * stride, C, Tn))
    ref, _ = _offline_power(rp, bins, coefs, [[7]])
    pipe.prime(bins[:, :win - stride])
    pipe.step(bins[:, win - stride:win])
    pipe.step(bins[:, win:])
    exp = cca.transform(pca.transform(ref[0, -win:])).astype(np.float32)
    got = pipe.features.cpu().numpy()[0]
    assert np.abs(got - exp).max() <= 1e-6 * np.abs(exp).max()


def _offline_logits(m, power, maps):
    """power (B, n_bins, C) -> map per stream -> float32 -> model forward (B, n_pred, ncls)."""
    xs = []
    for s in range(power.shape[0]):
        W, c = maps[s] if maps[s] is not None else (np.eye(power.shape[2]), np.zeros(power.shape[2]))
        xs.append((power[s] @ W + c).astype(np.float32))
    with torch.no_grad():
        return m(torch.from_numpy(np.stack(xs)).cuda())


@pytest.mark.parametrize('use_graph', [False, True])
@pytest.mark.parametrize('n_streams', [1, 3])
def test_end_to_end_vs_offline_composition_golden_size(use_graph, n_streams):
    """realtime_small.npz model shape (6 features, win 14, stride 4, H 32, L 2, 11 classes); 20 raw channels mapped to
    6 features by a different affine map per stream, different bad channels per stream."""
    rt, rp = _rt()
    from cross_patient_speech_decoding_amd.realtime_sim import greedy_decode_batch
    C, Tn, d, win, stride = 20, 40, 6, 14, 4
    m = _model(d, win, stride, H=32, L=2, ncls=11, seed=21)
    rng = np.random.default_rng(40 + n_streams)
    maps = [(rng.standard_normal((C, d)) * 3.0, rng.standard_normal(d) * 0.1) for _ in range(n_streams)]
    bads = [[0, 3], [], [19]][:n_streams]
    coefs = _iir(4, 2)
    pipe = rt.RealtimePipeline(m, coefs, C, Tn, n_streams=n_streams, bad_channels=bads, feature_map=maps,
                               use_graph=use_graph)
    n_bins = 62
    bins = rng.standard_normal((n_streams, n_bins, C, Tn))
    power, _ = _offline_power(rp, bins, coefs, bads)
    full = _offline_logits(m, power, maps)
    logits, dec = pipe.run(bins)
    assert logits.shape == full.shape == (n_streams, 13, 11)
    assert (logits - full).abs().max().item() <= 2e-5
    assert torch.equal(logits.argmax(-1), full.argmax(-1))
    ref = greedy_decode_batch(full, blank=0)
    for s in range(n_streams):
        assert torch.equal(dec[s], ref[s])
    # reset() + the same sequence: bitwise identical
    logits2, dec2 = pipe.run(bins)
    assert torch.equal(logits2, logits)
    for a, b in zip(dec, dec2):
        assert torch.equal(a, b)
    if n_streams == 3:                      # one stream's input changes; the others' outputs do not
        bins3 = bins.copy()
        bins3[1] = rng.standard_normal(bins3[1].shape)
        logits3, dec3 = pipe.run(bins3)
        for s in (0, 2):
            assert torch.equal(logits3[s], logits[s])
            assert torch.equal(dec3[s], dec[s])
        assert not torch.equal(logits3[1], logits[1])


def _config5_model():
    return _model(128, 14, 4, H=128, L=2, ncls=11, seed=505)


def test_end_to_end_config5_vs_offline_and_oracle():
    """Config 5 (128 channels x 40 samples, 8 IIR bands of order 4, win 14, stride 4, H 128, L 2, 11 classes), 200 bins
    -> 47 predictions: against the offline composition (2e-5, same tokens) and the CPU oracles (1e-4, same tokens)."""
    rt, rp = _rt()
    from oracle import realtime_processing_oracle as po
    from oracle.realtime_oracle import RealtimeOracle, greedy_decode_batch as greedy_ref
    from cross_patient_speech_decoding_amd.realtime_sim import greedy_decode_batch
    torch.set_num_threads(min(8, len(os.sched_getaffinity(0))))
    C, Tn, win, stride = 128, 40, 14, 4
    m = _config5_model()
    coefs = _iir(8, 4)
    bads = [[5, 77]]
    pipe = rt.RealtimePipeline(m, coefs, C, Tn, bad_channels=bads, use_graph=True)
    rng = np.random.default_rng(507)
    bins = rng.standard_normal((1, 200, C, Tn)) * 50.0
    power, _ = _offline_power(rp, bins, coefs, bads)
    full = _offline_logits(m, power, [None])
    logits, dec = pipe.run(bins)
    assert logits.shape == (1, 47, 11)
    assert (logits - full).abs().max().item() <= 2e-5
    assert torch.equal(logits.argmax(-1), full.argmax(-1))
    assert torch.equal(dec[0], greedy_decode_batch(full, blank=0)[0])
    # CPU oracles: scipy / numpy frontend, torch GRU
    ics, rows = None, []
    for j in range(200):
        p, ics = po.process_hg(bins[0, j], coefs, bad_channels=bads[0], filt_ics=ics)
        rows.append(p)
    x = torch.from_numpy(np.stack(rows)[None].astype(np.float32))
    orc = RealtimeOracle(win * C, 128, 2, 11, win, stride)
    orc.load_reference_state({k: v.detach().cpu() for k, v in m.state_dict().items()})
    orc.eval()
    with torch.no_grad():
        ref = orc(x)
    assert (logits.cpu() - ref).abs().max().item() <= 1e-4
    assert torch.equal(logits.argmax(-1).cpu(), ref.argmax(-1))
    np.testing.assert_array_equal(dec[0].cpu().numpy(), greedy_ref(torch.log_softmax(ref, -1))[0].numpy())


def test_errors():
    rt, _ = _rt()
    from cross_patient_speech_decoding_amd.realtime_sim import RealtimeRNNModel
    coefs = _iir(2, 2)
    C, Tn = 8, 20
    with pytest.raises(ValueError, match='unidirectional'):
        rt.RealtimePipeline(RealtimeRNNModel(14 * C, 8, 1, 5, bidirectional=True).cuda(), coefs, C, Tn)
    with pytest.raises(RuntimeError, match='no CPU fallback'):
        rt.RealtimePipeline(RealtimeRNNModel(14 * C, 8, 1, 5), coefs, C, Tn)
    with pytest.raises(ValueError, match='win_size'):
        rt.RealtimePipeline(_model(C + 1, 14, 4), coefs, C, Tn)
    with pytest.raises(ValueError, match='stride'):
        rt.RealtimePipeline(_model(C, 3, 4), coefs, C, Tn)
    with pytest.raises(ValueError, match='streams'):
        rt.RealtimePipeline(_model(C, 6, 4), coefs, C, Tn, n_streams=9)
    pipe = rt.RealtimePipeline(_model(C, 6, 4, ncls=3), coefs, C, Tn, max_tokens=1, use_graph=False)
    with pytest.raises(ValueError, match='bins of shape'):
        pipe.prime(np.zeros((1, 3, C, Tn)))
    with pytest.raises(RuntimeError, match='prime'):
        pipe.step(np.zeros((1, 4, C, Tn)))
    pipe.prime(np.zeros((1, 2, C, Tn)))
    with pytest.raises(ValueError, match='bins of shape'):
        pipe.step(np.zeros((1, 4, C, Tn + 1)))
    # token overflow: force alternating argmaxes through the classifier bias
    with torch.no_grad():
        fc = pipe.model.classifier.fc
        fc.weight.zero_()
    for cls in (1, 2, 1):
        with torch.no_grad():
            pipe._fc[1].fill_(0.0)
            pipe._fc[1][cls] = 1.0
        pipe.step(np.zeros((1, 4, C, Tn)))
        assert int(pipe.token[0]) == cls
    with pytest.raises(RuntimeError, match='max_tokens'):
        pipe.decoded(0)
    pipe.reset()
    assert pipe.decoded(0).numel() == 0


def test_latency_config5_batch1():
    """Per-prediction latency at the config-5 shape, batch 1: pinned bins -> H2D -> graph replay -> D2H of logits and
    token -> synchronise.  Loose bar: the reference's 2.06 ms per prediction (other hardware, host transform)."""
    rt, _ = _rt()
    C, Tn = 128, 40
    pipe = rt.RealtimePipeline(_config5_model(), _iir(8, 4), C, Tn)
    bins = torch.from_numpy(np.random.default_rng(9).standard_normal((1, 4, C, Tn))).pin_memory()
    out_l = torch.empty(1, 11).pin_memory()
    out_t = torch.empty(1, dtype=torch.int64).pin_memory()
    pipe.prime(np.zeros((1, 10, C, Tn)))
    ts = []
    for i in range(300):
        t0 = time.perf_counter()
        pipe.step(bins)
        out_l.copy_(pipe.logits, non_blocking=True)
        out_t.copy_(pipe.token, non_blocking=True)
        torch.cuda.synchronize()
        ts.append(time.perf_counter() - t0)
    med = float(np.median(ts[50:])) * 1e6
    print(f'realtime pipeline per-prediction latency (config 5, batch 1, H2D + replay + D2H): median {med:.1f} us')
    assert med < 2060.0
