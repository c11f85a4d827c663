"""Session replay as the producer of the CTC data modules' input, and back: the features of two synthetic patients (12 and
10 electrodes) go into a CTCHeldOutTargetValAlignDataModule, and the module's own feature_maps(), given to one SessionReplay
over both patients' raw trials, reproduce the module's un-augmented training rows."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from weights import weights_from_seed  # noqa: E402

N_BINS, TN, N_COMP, WIN, STRIDE = 30, 40, 6, 4, 2
BAD = ([1], [3])                      # bad electrodes of the target and of the cross patient


def _iir(nb, order):
    import scipy.signal as signal
    out = []
    for k in range(nb):
        b, a = signal.butter(order, [60 + 12 * k, 72 + 12 * k], btype='band', fs=2000)
        out.append(np.stack([a, b], axis=1))
    return np.stack(out)


def _model(C_in):
    from cross_patient_speech_decoding_amd.realtime_sim import RealtimeRNNModel
    m = RealtimeRNNModel(WIN * C_in, 16, 1, 7, dropout=0.0, win_size=WIN, stride=STRIDE)
    m.load_state_dict(weights_from_seed(m.state_dict(), 4))
    return m.cuda().eval()


def _two_patients():
    """Raw trials whose band power carries three phoneme segments per trial through a patient-specific mixing: the task of
    tests/test_gpu_ctc_data.py's three patients, as amplitudes of white noise.  Six label sequences shared by both."""
    rng = np.random.default_rng(2025)
    seqs = np.array([[1, 2, 3], [2, 4, 1], [3, 5, 2], [4, 1, 5], [5, 3, 4], [2, 2, 5]])
    proto = rng.standard_normal((6, 4))
    out = []
    for n, C in ((40, 12), (32, 10)):
        lab = seqs[rng.permutation(n) % len(seqs)]
        z = 0.3 * rng.standard_normal((n, N_BINS, 4))
        for j in range(3):
            z[:, 3 + 8 * j:11 + 8 * j] += proto[lab[:, j]][:, None, :]
        amp = 20.0 * np.exp(0.5 * (z @ (rng.standard_normal((4, C)) / 2)))
        out.append((rng.standard_normal((n, N_BINS, C, TN)) * amp[..., None], lab.astype(np.int64)))
    return out


def _cpu_power(raw, coefs, bad):
    from oracle import realtime_processing_oracle as po
    out = np.empty(raw.shape[:3])
    for n in range(raw.shape[0]):
        ics = None
        for j in range(raw.shape[1]):
            out[n, j], ics = po.process_hg(raw[n, j], coefs, bad_channels=bad, filt_ics=ics)
    return out


def _cpu_one_stage_vs_two_stage(x_t, y_t, x_c, y_c):
    """numpy on the CPU, this test's own data: x (float64 band power from the CPU oracle) through the folded one-stage map
    x @ W + c against the module's two-stage path on float32(x) with a float32 rounding after each stage (exact PCA, the
    CCA oracle).  Max over the target's and the cross patient's rows."""
    from oracle.align_oracle import AlignCCAOracle, pca_exact

    def reduce(x):
        x32 = x.astype(np.float32).astype(np.float64)
        mean, comps, _ = pca_exact(x32.reshape(-1, x.shape[-1]), N_COMP)
        return mean, comps, ((x32 - mean) @ comps.T).astype(np.float32)

    mean_t, comps_t, red_t = reduce(x_t)
    worst = np.abs(x_t @ comps_t.T - mean_t @ comps_t.T - red_t).max()
    mean_c, comps_c, red_c = reduce(x_c)
    al = AlignCCAOracle().fit(red_t.astype(np.float64), red_c.astype(np.float64), y_t, y_c)
    M = al.M_b @ np.linalg.pinv(al.M_a)
    two = (red_c.astype(np.float64) @ M).astype(np.float32)
    W = comps_c.T @ M
    return max(worst, np.abs(x_c @ W - mean_c @ W - two).max())


def test_feature_maps_of_the_module_reproduce_its_training_rows_from_raw_trials():
    """The bound is derived as tests/test_gpu_ctc_data.py::test_feature_maps_reproduce_the_aligned_training_rows derives
    it: the one-stage versus two-stage discrepancy of this test's own data, computed with numpy on the CPU (float32
    roundings between the module's stages, and of its input), times 4 for the module's two further roundings and its
    different order of operations.  No literal."""
    from cross_patient_speech_decoding_amd.realtime_sim import CTCHeldOutTargetValAlignDataModule, SessionReplay
    coefs = _iir(4, 2)
    (raw_t, y_t), (raw_c, y_c) = _two_patients()
    C = raw_t.shape[2]
    rng = np.random.default_rng(7)
    order = rng.permutation(len(raw_t))
    tr, va = order[:30], order[30:]
    bound = 4 * _cpu_one_stage_vs_two_stage(_cpu_power(raw_t[tr], coefs, BAD[0]), y_t[tr],
                                            _cpu_power(raw_c, coefs, BAD[1]), y_c)

    # producer: each patient's recordings -> features (identity map: the float32 band power), on its own electrodes
    feats = []
    for raw, bad in ((raw_t, BAD[0]), (raw_c, BAD[1])):
        f = SessionReplay(_model(raw.shape[2]), coefs, raw.shape[2], TN, bad_channels=bad).features(raw)
        assert f.dtype == torch.float32 and f.shape == raw.shape[:3]
        feats.append(f.cpu())
    dm = CTCHeldOutTargetValAlignDataModule(feats[0], y_t, [feats[1]], [y_c], feats[0][va], y_t[va], val_size=0.25,
                                            n_comp=N_COMP, split_indices=(tr, va))
    dm.setup()
    maps = dm.feature_maps()
    assert len(maps) == 2 and maps[0][0].shape == (C, N_COMP) and maps[1][0].shape == (raw_c.shape[2], N_COMP)

    # and back: one replay over both patients with the module's maps; the patient with fewer electrodes is padded with
    # bad channels and zero rows of W
    pad = C - raw_c.shape[2]
    W_c = np.concatenate([maps[1][0], np.zeros((pad, N_COMP))])
    raw_c_pad = np.concatenate([raw_c, np.zeros(raw_c.shape[:2] + (pad, TN))], axis=2)
    replay = SessionReplay(_model(N_COMP), coefs, C, TN, bad_channels=[BAD[0], BAD[1] + list(range(C - pad, C))],
                           feature_map=[maps[0], (W_c, maps[1][1])])
    raw_all = np.concatenate([raw_t[tr], raw_c_pad])
    patient = np.array([0] * len(tr) + [1] * len(raw_c))
    got = replay.features(raw_all, patient=patient).cpu().numpy().astype(np.float64)
    rows = dm._folds[0]['train_data'].cpu().numpy().astype(np.float64)
    assert rows.shape == got.shape == (len(tr) + len(raw_c), N_BINS, N_COMP)       # no augmentation: the two slabs only
    err_t = np.abs(got[:len(tr)] - rows[:len(tr)]).max()
    err_c = np.abs(got[len(tr):] - rows[len(tr):]).max()
    print('hand-off: max abs err target', err_t, 'cross', err_c, 'bound', bound, 'row scale', np.abs(rows).max())
    assert err_t <= bound and err_c <= bound
    # the same maps serve the run: logits of the replayed session come from exactly these rows
    res = replay.run(raw_all, patient=patient)
    assert torch.equal(res.features.cpu(), torch.from_numpy(got.astype(np.float32)))
