"""Cross-patient CTC data path on the MI355X: per-trial augmentation kernels, batched greedy decode, batched edit distance,
reduce_to_latent_space / align_to_target / the data modules against the reference's recorded results
(tests/golden/ctc_data.npz, written by tests/golden/make_ctc_data_fixtures.py), feature_maps() and an end-to-end training run."""
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(__file__), 'golden')


@pytest.fixture(scope='module')
def g():
    return dict(np.load(os.path.join(GOLDEN, 'ctc_data.npz')))


def _aug():
    from cross_patient_speech_decoding_amd.realtime_sim import augmentations as A
    return A


def _lib_call(name, *args):
    from cross_patient_speech_decoding_amd._lib import call
    call(name, *args, torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()


# ---- torch CPU expressions of the reference ---------------------------------------------------------------------------------
def ref_shift(x, shifts):
    B, T, _ = x.shape
    idx = (torch.arange(T)[None, :] - shifts[:, None]) % T
    return x[torch.arange(B).unsqueeze(1), idx]


def ref_mask(x, starts, size):
    out = x.clone()
    for i in range(len(x)):
        out[i, starts[i]:starts[i] + size] = 0
    return out


def ref_warp(x, T2):
    T = x.shape[1]
    rows = []
    for i in range(len(x)):
        v = x[i].unsqueeze(0).transpose(1, 2)
        v = F.interpolate(v, size=int(T2[i]), mode='linear', align_corners=False)
        v = F.interpolate(v, size=T, mode='linear', align_corners=False)
        rows.append(v.transpose(1, 2).squeeze(0))
    return torch.stack(rows)


def levenshtein(a, b):
    prev = list(range(len(b) + 1))
    for i, x in enumerate(a, 1):
        cur = [i]
        for j, y in enumerate(b, 1):
            cur.append(min(prev[j] + 1, cur[j - 1] + 1, prev[j - 1] + (x != y)))
        prev = cur
    return prev[-1]


def ref_greedy(log_probs, blank=0):
    best = log_probs.argmax(dim=2)
    keep = torch.ones_like(best, dtype=torch.bool)
    keep[:, 1:] = best[:, 1:] != best[:, :-1]
    keep &= best != blank
    return [best[b][keep[b]] for b in range(best.size(0))]


# ---- augmentations -----------------------------------------------------------------------------------------------------------
def test_augmentations_reproduce_the_reference_on_a_host_tensor(g):
    """Host tensor + torch.manual_seed: same draws as the reference, results back on the host.  Shift / mask / scale / jitter
    bit-exact, warp within the bar tests/test_gpu_augmentations.py sets for the existing warp."""
    A = _aug()
    x = torch.from_numpy(g['aug_x'])
    seeds = dict(zip(('warp', 'mask', 'shift', 'jitter', 'scale'), (int(s) for s in g['aug_seeds'])))
    for name, fn in (('mask', A.time_masking), ('shift', A.time_shifting), ('jitter', A.noise_jitter), ('scale', A.scaling)):
        torch.manual_seed(seeds[name])
        out = fn(x)
        assert not out.is_cuda and out.dtype == torch.float32
        assert np.array_equal(out.numpy(), g[f'aug_{name}']), name
    torch.manual_seed(seeds['warp'])
    out = A.time_warping(x)
    err = np.abs(out.numpy() - g['aug_warp']).max()
    print('warp vs golden: max abs err', err)
    np.testing.assert_allclose(out.numpy(), g['aug_warp'], rtol=0, atol=2e-6)


@pytest.mark.parametrize('shape', [(10, 60, 8), (7, 200, 128), (5, 33, 7), (4, 50, 10)])
def test_kernels_against_the_torch_cpu_expression_for_fresh_draws(shape):
    N, T, C = shape
    rng = np.random.default_rng(N * 1000 + C)
    x = torch.from_numpy(rng.standard_normal(shape).astype(np.float32))
    xd = x.cuda()
    shifts = torch.from_numpy(rng.integers(-T - 5, T + 6, N))
    starts = torch.from_numpy(rng.integers(0, T - T // 10 + 1, N))
    scales = torch.from_numpy(rng.uniform(0.9, 1.1, N).astype(np.float32))
    T2 = torch.from_numpy(rng.integers(int(0.8 * T), int(1.2 * T) + 1, N))
    T2[0], T2[-1] = T, 1
    noise = torch.from_numpy(rng.standard_normal(shape).astype(np.float32))
    # outputs are slabs of one larger buffer, as the data modules use the kernels
    buf = torch.full((5 * N + 1, T, C), 7.0, device='cuda')
    _lib_call('xps_aug_trial_shift_f32', xd.data_ptr(), buf[0:N].data_ptr(), N, T, C, shifts.cuda().data_ptr())
    _lib_call('xps_aug_trial_mask_f32', xd.data_ptr(), buf[N:2 * N].data_ptr(), N, T, C, starts.cuda().data_ptr(), T // 10)
    _lib_call('xps_aug_trial_scale_f32', xd.data_ptr(), buf[2 * N:3 * N].data_ptr(), N, T * C, scales.cuda().data_ptr())
    _lib_call('xps_aug_jitter_f32', xd.data_ptr(), noise.cuda().data_ptr(), buf[3 * N:4 * N].data_ptr(), x.numel(), 0.01)
    _lib_call('xps_aug_trial_warp_f32', xd.data_ptr(), buf[4 * N:5 * N].data_ptr(), N, T, C, T2.cuda().data_ptr())
    out = buf.cpu()
    assert torch.equal(out[0:N], ref_shift(x, shifts))
    assert torch.equal(out[N:2 * N], ref_mask(x, starts, T // 10))
    assert torch.equal(out[2 * N:3 * N], x * scales[:, None, None])
    assert torch.equal(out[3 * N:4 * N], x + noise * 0.01)
    ref = ref_warp(x, T2)
    print(shape, 'warp max abs err', (out[4 * N:5 * N] - ref).abs().max().item())
    np.testing.assert_allclose(out[4 * N:5 * N].numpy(), ref.numpy(), rtol=0, atol=2e-6)
    assert torch.all(out[5 * N] == 7.0)                                # nothing written past the last slab


def test_identity_draws_return_the_input_bit_exact():
    A = _aug()
    rng = np.random.default_rng(5)
    x = torch.from_numpy(rng.standard_normal((6, 40, 12)).astype(np.float32)).cuda()
    assert torch.equal(A.time_shifting(x, shift_max=0), x)
    assert torch.equal(A.time_warping(x, factor_range=(1.0, 1.0)), x)
    assert torch.equal(A.scaling(x, scale_range=(1.0, 1.0)), x)
    assert torch.equal(A.time_masking(x, mask_ratio=0.0), x)
    out = torch.empty_like(x)
    assert A.time_shifting(x, shift_max=0, out=out) is out and torch.equal(out, x)


def test_device_tensors_stay_on_the_device_and_draw_there():
    A = _aug()
    x = torch.randn(8, 50, 8, device='cuda')
    torch.manual_seed(21)
    a = A.time_shifting(x)
    torch.manual_seed(21)
    shifts = A.draw_shifts(8, x.device)
    assert a.is_cuda and shifts.is_cuda
    assert torch.equal(a.cpu(), ref_shift(x.cpu(), shifts.cpu()))


# ---- decode ------------------------------------------------------------------------------------------------------------------
def _check_decode(logits_btc, blank=0):
    from cross_patient_speech_decoding_amd.realtime_sim import greedy_decode_batch, greedy_decode_device
    ref = ref_greedy(logits_btc, blank)
    d = logits_btc.cuda()
    got = greedy_decode_batch(d, blank=blank)                                        # batch-major
    assert len(got) == len(ref)
    for a, b in zip(got, ref):
        assert a.is_cuda and a.dtype == torch.int64 and torch.equal(a.cpu(), b)
    tm = d.permute(1, 0, 2).contiguous()                                             # time-major storage
    tokens, lengths = greedy_decode_device(tm, blank=blank, time_major=True)
    view_tokens, view_lengths = greedy_decode_device(tm.permute(1, 0, 2), blank=blank)   # (B, T, C) view of it: strides only
    assert torch.equal(tokens, view_tokens) and torch.equal(lengths, view_lengths)
    assert lengths.tolist() == [len(r) for r in ref]
    for b, r in enumerate(ref):
        assert torch.equal(tokens[b, :len(r)].cpu(), r)
        assert torch.all(tokens[b, len(r):] == -1)


def test_greedy_decode_kernel_matches_the_cpu_expression():
    rng = np.random.default_rng(11)
    B, T, C = 37, 150, 9
    logits = rng.standard_normal((B, T, C)).astype(np.float32)
    for b in range(B):                                   # forced repeats and blanks
        for t in range(1, T):
            u = rng.random()
            if u < 0.35:
                logits[b, t] = logits[b, t - 1]
            elif u < 0.55:
                logits[b, t, 0] = 9.0
    logits[3, 10, 2] = logits[3, 10, 5] = 20.0           # an exact tie: lowest index
    _check_decode(torch.from_numpy(logits))
    _check_decode(torch.from_numpy(logits), blank=4)
    _check_decode(torch.from_numpy(logits.astype(np.float64)))
    _check_decode(torch.from_numpy(logits[:1]))                                       # B = 1
    _check_decode(torch.from_numpy(logits[:, :1]))                                    # T = 1
    allblank = logits.copy()
    allblank[..., 0] = 50.0
    _check_decode(torch.from_numpy(allblank))                                         # all frames blank


def test_greedy_decode_kernel_on_the_golden_decodes():
    from cross_patient_speech_decoding_amd.realtime_sim import greedy_decode_batch
    r = np.load(os.path.join(GOLDEN, 'realtime_small.npz'))
    logits = torch.from_numpy(r['logits'])
    dec = greedy_decode_batch(torch.log_softmax(logits, -1).cuda(), blank=0)
    for i, d in enumerate(dec):
        assert np.array_equal(d.cpu().numpy(), r[f'dec{i}'])


# ---- edit distance -----------------------------------------------------------------------------------------------------------
def _distances(pairs):
    from cross_patient_speech_decoding_amd.realtime_sim import edit_distance_device
    P = max(max(len(a) for a, _ in pairs), 1)
    L = max(max(len(b) for _, b in pairs), 1)
    pred = torch.full((len(pairs), P), -7, dtype=torch.int64)
    tgt = torch.full((len(pairs), L), -9, dtype=torch.int64)
    for i, (a, b) in enumerate(pairs):
        pred[i, :len(a)] = torch.tensor(a, dtype=torch.int64)
        tgt[i, :len(b)] = torch.tensor(b, dtype=torch.int64)
    out = edit_distance_device(pred.cuda(), torch.tensor([len(a) for a, _ in pairs]), tgt.cuda(),
                               torch.tensor([len(b) for _, b in pairs]))
    assert out.is_cuda and out.dtype == torch.int64
    return out.tolist()


def test_edit_distance_kernel_matches_a_plain_levenshtein():
    rng = np.random.default_rng(17)
    pairs = []
    for _ in range(60):                                   # random pairs, lengths 0..300, small alphabet (many matches)
        la, lb = int(rng.integers(0, 301)), int(rng.integers(0, 301))
        pairs.append((rng.integers(1, 5, la).tolist(), rng.integers(1, 5, lb).tolist()))
    pairs.append(([], [1, 2, 3]))                         # an empty prediction
    pairs.append(([4, 4, 1], []))                         # an empty target
    pairs.append(([], []))
    same = rng.integers(1, 40, 200).tolist()
    pairs.append((same, list(same)))                      # equal sequences
    for n in (63, 64, 65, 127, 128, 129):                 # the 64-column chunk boundary
        for m in (1, 63, 64, 65, 100):
            pairs.append((rng.integers(1, 4, m).tolist(), rng.integers(1, 4, n).tolist()))
    assert _distances(pairs) == [levenshtein(a, b) for a, b in pairs]
    short = [(a[:40], b[:50]) for a, b in pairs[:30]]     # the one-chunk kernel
    assert _distances(short) == [levenshtein(a, b) for a, b in short]


def test_edit_distance_of_a_4096_token_prediction():
    rng = np.random.default_rng(19)
    pairs = [(rng.integers(1, 6, 4096).tolist(), rng.integers(1, 6, 256).tolist()),
             (rng.integers(1, 6, 4096).tolist(), rng.integers(1, 6, 3).tolist()),
             (rng.integers(1, 6, 1000).tolist(), rng.integers(1, 6, 1024).tolist())]
    assert _distances(pairs) == [levenshtein(a, b) for a, b in pairs]


def test_edit_distance_beyond_the_supported_sizes_raises():
    from cross_patient_speech_decoding_amd.realtime_sim import edit_distance_device
    one = torch.ones(1, dtype=torch.int64)
    with pytest.raises(ValueError):
        edit_distance_device(torch.zeros(1, 3, dtype=torch.int64, device='cuda'), one, torch.zeros(1, 1025, dtype=torch.int64,
                                                                                                device='cuda'), one)
    with pytest.raises(ValueError):
        edit_distance_device(torch.zeros(1, 65537, dtype=torch.int64, device='cuda'), one, torch.zeros(1, 3, dtype=torch.int64,
                                                                                                 device='cuda'), one)


def test_scalar_wrappers_and_calc_per_keep_their_values():
    from cross_patient_speech_decoding_amd.realtime_sim import calc_PER, edit_distance
    assert edit_distance([1, 2, 3, 4], [1, 3, 4, 4, 5]) == levenshtein([1, 2, 3, 4], [1, 3, 4, 4, 5])
    assert edit_distance(torch.tensor([2, 2]), torch.tensor([], dtype=torch.int64)) == 2
    decoded = [torch.tensor([1, 2, 3]), torch.tensor([], dtype=torch.int64), torch.tensor([5, 5, 1, 2])]
    targets = torch.tensor([[1, 2, 4], [3, 3, 0], [5, 1, 2]])
    lengths = torch.tensor([3, 2, 3])
    want = sum(levenshtein(p.tolist(), t[:l].tolist()) for p, t, l in zip(decoded, targets, lengths)) / 8.0 * 100
    assert calc_PER(decoded, targets, lengths) == want
    assert calc_PER([d.cuda() for d in decoded], targets.cuda(), lengths.cuda()) == want


def test_validation_step_reproduces_the_golden_per_with_one_scalar_on_the_device():
    import sys
    sys.path.insert(0, GOLDEN)
    from weights import weights_from_seed
    from cross_patient_speech_decoding_amd.realtime_sim import RealtimeRNNModel, calc_PER, greedy_decode_batch
    r = np.load(os.path.join(GOLDEN, 'realtime_train_small.npz'))
    C, win, stride, H, Lr, ncls = (int(v) for v in r['cfg'])
    m = RealtimeRNNModel(win * C, H, Lr, ncls, dropout=0.0, win_size=win, stride=stride)
    sd = weights_from_seed(m.state_dict(), int(r['seed']))
    sd['h0'] = torch.from_numpy(r['h0'])
    m.load_state_dict(sd)
    m.cuda().eval()
    batch = tuple(torch.from_numpy(r[k]).cuda() for k in ('x', 'targets', 'input_lengths', 'target_lengths'))
    with torch.no_grad():
        m.validation_step(batch, 0)
        per = m._xps_logged['val_PER']
        assert torch.is_tensor(per) and per.is_cuda and per.dim() == 0            # the transfer is the caller's float()
        np.testing.assert_allclose(float(per), float(r['val_PER']), rtol=1e-6)
        dec = greedy_decode_batch(m(batch[0]), blank=0)
    np.testing.assert_allclose(calc_PER(dec, batch[1], batch[3]), float(r['val_PER']), rtol=1e-6)


# ---- reduce / align / data modules ---------------------------------------------------------------------------------------------
TOL = 2e-4          # tests/test_gpu_training.py: process_aligner against its oracle composition, float32 data


def _close_up_to_column_sign(got, want, comps_got, comps_want):
    """PCA columns are defined up to sign: where this fit's component has the other sign than the golden's, flip the column."""
    signs = np.sign(np.sum(comps_got * comps_want, axis=1))
    np.testing.assert_allclose(got * signs, want, rtol=0, atol=TOL)


def test_reduce_to_latent_space_against_the_reference(g):
    from cross_patient_speech_decoding_amd.alignment import PCA
    from cross_patient_speech_decoding_amd.realtime_sim import reduce_to_latent_space
    x = torch.from_numpy(g['pt_tgt'])
    out, pca = reduce_to_latent_space(x, n_components=6)
    assert isinstance(pca, PCA) and pca.n_components_ == 6
    assert out.dtype == torch.float32 and not out.is_cuda and out.shape == g['red_fit'].shape
    np.testing.assert_allclose(pca.mean_, g['red_mean'], rtol=0, atol=TOL)
    _close_up_to_column_sign(out.numpy(), g['red_fit'], pca.components_, g['red_components'])
    dev, _ = reduce_to_latent_space(torch.from_numpy(g['red_x2']).cuda(), pca=pca)       # transform with a given PCA; stays on the device
    assert dev.is_cuda and dev.dtype == torch.float32
    _close_up_to_column_sign(dev.cpu().numpy(), g['red_transform'], pca.components_, g['red_components'])
    wide, pca_w = reduce_to_latent_space(torch.from_numpy(g['red_wide']), n_components=4)   # 4 <= low_thresh: re-fit with 30
    assert pca_w.n_components_ == 30 and wide.shape == g['red_refit'].shape
    # 120 samples of rank-4 signal + noise in 32 channels: the trailing components are well separated noise directions
    _close_up_to_column_sign(wide.numpy(), g['red_refit'], pca_w.components_, g['red_refit_components'])


def test_align_to_target_against_the_reference(g):
    from cross_patient_speech_decoding_amd.alignment import AlignCCA
    from cross_patient_speech_decoding_amd.realtime_sim import align_to_target
    tgt, src = torch.from_numpy(g['red_fit']), torch.from_numpy(g['align_src'])
    out = align_to_target(AlignCCA, tgt, src, torch.from_numpy(g['pt_tgt_labels']), torch.from_numpy(g['align_src_labels']))
    assert out.dtype == torch.float32 and out.shape == g['align_out'].shape
    np.testing.assert_allclose(out.numpy(), g['align_out'], rtol=0, atol=TOL)
    dev = align_to_target(AlignCCA, tgt.cuda(), src.cuda(), torch.from_numpy(g['pt_tgt_labels']),
                          torch.from_numpy(g['align_src_labels']))
    assert dev.is_cuda
    np.testing.assert_allclose(dev.cpu().numpy(), g['align_out'], rtol=0, atol=TOL)


def _module_args(g):
    return (g['pt_tgt'], g['pt_tgt_labels'], [g['pt_cross0'], g['pt_cross1']], [g['pt_cross0_labels'], g['pt_cross1_labels']],
            g['pt_test'], g['pt_test_labels'])


def _check_fold(fold, g, prefix):
    for k in ('train', 'val', 'test'):
        data, labels = fold[f'{k}_data'], fold[f'{k}_labels']
        assert data.is_cuda and data.dtype == torch.float32 and labels.dtype == torch.int64
        assert np.array_equal(labels.cpu().numpy(), g[f'{prefix}_{k}_labels']), k
        err = np.abs(data.cpu().numpy() - g[f'{prefix}_{k}_data']).max()
        print(prefix, k, tuple(data.shape), 'max abs err', err)
        np.testing.assert_allclose(data.cpu().numpy(), g[f'{prefix}_{k}_data'], rtol=0, atol=TOL)


def test_full_setup_matches_every_dataset_of_the_golden(g, tmp_path):
    """Recorded split_indices + the same seeds: labels exactly, data to 2e-4; rows in the reference's order (target, cross
    patients, then one augmented copy per augmentation).  The target PCA's signs are the golden's (same sign rule)."""
    A = _aug()
    from cross_patient_speech_decoding_amd.realtime_sim import CTCHeldOutTargetValAlignDataModule
    np.random.seed(int(g['ho_seeds'][0]))
    torch.manual_seed(int(g['ho_seeds'][1]))
    dm = CTCHeldOutTargetValAlignDataModule(*_module_args(g), batch_size=-1, val_size=float(g['val_size']),
                                            augmentations=[A.time_shifting, A.scaling], data_path=tmp_path,
                                            n_comp=int(g['n_comp']), split_indices=(g['ho_train_idx'], g['ho_val_idx']),
                                            save_folds=True)
    dm.setup()
    _check_fold(dm._folds[0], g, 'ho')
    assert dm.get_data_shape() == g['ho_train_data'].shape
    n_pool = len(g['ho_train_idx']) + len(g['pt_cross0']) + len(g['pt_cross1'])
    assert dm.get_data_shape()[0] == 3 * n_pool
    batches = list(dm.train_dataloader())
    assert len(batches) == 1 and all(t.is_cuda for t in batches[0])
    x, y, il, tl = batches[0]
    assert x.shape == g['ho_train_data'].shape and y.shape == g['ho_train_labels'].shape
    assert il.tolist() == [x.shape[1]] * len(x) and tl.tolist() == [3] * len(x)
    vx, vy, _, _ = next(iter(dm.val_dataloader()))
    assert torch.equal(vx, dm._folds[0]['val_data']) and torch.equal(vy, dm._folds[0]['val_labels'])
    with np.load(tmp_path / 'rnn_realtime.npz') as f:                  # the cache carries the reference's dataset names
        assert sorted(f.files) == sorted(['train_data', 'train_labels', 'val_data', 'val_labels', 'test_data', 'test_labels'])
        assert np.array_equal(f['train_data'], dm._folds[0]['train_data'].cpu().numpy())


def test_default_split_draws_what_the_reference_draws(g):
    """Without split_indices the split comes from numpy's global generator exactly as in the reference."""
    from cross_patient_speech_decoding_amd.realtime_sim import CTCHeldOutTargetValAlignDataModule
    np.random.seed(int(g['ho_seeds'][0]))
    dm = CTCHeldOutTargetValAlignDataModule(*_module_args(g), val_size=float(g['val_size']), n_comp=int(g['n_comp']))
    (tr, va), = dm._splits()
    assert np.array_equal(tr, g['ho_train_idx']) and np.array_equal(va, g['ho_val_idx'])


def test_cv_fold_matches_the_golden(g):
    A = _aug()
    from cross_patient_speech_decoding_amd.realtime_sim import CTCHeldOutTargetValAlignCVDataModule
    np.random.seed(int(g['cv_seeds'][0]))
    torch.manual_seed(int(g['cv_seeds'][1]))
    folds = int(g['cv_folds'])
    dm = CTCHeldOutTargetValAlignCVDataModule(*_module_args(g), batch_size=16, n_folds=folds,
                                              augmentations=[A.time_shifting, A.scaling], n_comp=int(g['n_comp']),
                                              split_indices=[(g[f'cv_train_idx{f}'], g[f'cv_val_idx{f}']) for f in range(folds)])
    dm.setup()
    assert sorted(dm._folds) == list(range(folds))
    _check_fold(dm._folds[0], g, 'cv')
    dm.set_fold(2)
    assert sum(len(b[0]) for b in dm.train_dataloader()) == dm.get_data_shape()[0]
    np.random.seed(int(g['cv_seeds'][0]))                              # the unpinned folds are the reference's too
    dm2 = CTCHeldOutTargetValAlignCVDataModule(*_module_args(g), n_folds=folds, n_comp=int(g['n_comp']))
    for f, (tr, va) in enumerate(dm2._splits()):
        assert np.array_equal(tr, g[f'cv_train_idx{f}']) and np.array_equal(va, g[f'cv_val_idx{f}'])


def test_plain_modules_pool_and_split(g):
    """The three modules without alignment: rows = target split (+ cross rows as given) (+ augmented copies)."""
    A = _aug()
    from cross_patient_speech_decoding_amd.realtime_sim import (CTCHeldOutDataModule, CTCHeldOutTargetValCVDataModule,
                                                                CTCHeldOutTargetValDataModule)
    x, y = g['pt_tgt'], g['pt_tgt_labels']
    tr, va = g['ho_train_idx'], g['ho_val_idx']
    dm = CTCHeldOutDataModule(x, y, g['pt_test'], g['pt_test_labels'], batch_size=5, augmentations=[A.scaling],
                              split_indices=(tr, va))
    torch.manual_seed(4)
    dm.setup()
    f = dm._folds[0]
    assert np.array_equal(f['train_data'][:len(tr)].cpu().numpy(), x[tr]) and np.array_equal(f['val_data'].cpu().numpy(), x[va])
    torch.manual_seed(4)
    scales = A.draw_scales(len(tr), 'cpu')
    assert torch.equal(f['train_data'][len(tr):].cpu(), torch.from_numpy(x[tr]) * scales)
    assert np.array_equal(f['train_labels'].cpu().numpy(), np.concatenate([y[tr], y[tr]]))
    extra, extra_y = x[:6] * 2, y[:6]
    dm = CTCHeldOutTargetValDataModule(x, y, extra, extra_y, g['pt_test'], g['pt_test_labels'], val_size=0, split_indices=None)
    dm.setup()
    assert dm.val_dataloader() is None
    assert np.array_equal(dm._folds[0]['train_data'].cpu().numpy(), np.concatenate([x, extra]))
    dm = CTCHeldOutTargetValCVDataModule(x, y, extra, extra_y, g['pt_test'], g['pt_test_labels'], n_folds=3,
                                         split_indices=[(g[f'cv_train_idx{k}'], g[f'cv_val_idx{k}']) for k in range(3)])
    dm.setup()
    dm.set_fold(1)
    assert np.array_equal(dm._folds[1]['train_data'].cpu().numpy(), np.concatenate([x[g['cv_train_idx1']], extra]))
    assert np.array_equal(next(iter(dm.val_dataloader()))[1].cpu().numpy(), y[g['cv_val_idx1']])


def _cpu_feature_map_discrepancy(g):
    """numpy on the CPU, from the golden alone: max |x_raw @ W + c - the reference's aligned training rows| over both cross
    patients, W, c folded from an exact PCA and the CCA oracle fitted on the golden's own (float32) stages."""
    from oracle.align_oracle import AlignCCAOracle, pca_exact
    ntr = len(g['ho_train_idx'])
    tgt, yt = g['ho_train_data'][:ntr].astype(np.float64), g['ho_train_labels'][:ntr]
    at, worst = ntr, 0.0
    for j in (0, 1):
        x, y = g[f'pt_cross{j}'].astype(np.float64), g[f'pt_cross{j}_labels']
        mean, comps, _ = pca_exact(x.reshape(-1, x.shape[-1]), int(g['n_comp']))
        red = ((x - mean) @ comps.T).astype(np.float32)
        al = AlignCCAOracle().fit(tgt, red.astype(np.float64), yt, y)
        W = comps.T @ al.M_b @ np.linalg.pinv(al.M_a)
        c = -mean @ W
        worst = max(worst, np.abs(x @ W + c - g['ho_train_data'][at:at + len(x)]).max())
        at += len(x)
    return worst


def test_feature_maps_reproduce_the_aligned_training_rows(g):
    """feature_maps(): raw cross-patient trials through x @ W + c against the module's own aligned training rows.  The one-stage
    map and the two-stage path differ by the float32 roundings between the reference's stages; the same two quantities
    computed with numpy from the golden differ by 7.4e-07 (rows up to 16 in magnitude: half an ulp there is 9.5e-07), and
    the module is allowed 4x that: its two-stage path rounds twice more and its order of operations differs."""
    from cross_patient_speech_decoding_amd.realtime_sim import CTCHeldOutTargetValAlignDataModule
    bound = 4 * _cpu_feature_map_discrepancy(g)
    dm = CTCHeldOutTargetValAlignDataModule(*_module_args(g), val_size=float(g['val_size']), n_comp=int(g['n_comp']),
                                            split_indices=(g['ho_train_idx'], g['ho_val_idx']))
    dm.setup()
    maps = dm.feature_maps()
    assert len(maps) == 3
    rows = dm._folds[0]['train_data'].cpu().numpy().astype(np.float64)
    ntr = len(g['ho_train_idx'])
    raw = [g['pt_tgt'][g['ho_train_idx']], g['pt_cross0'], g['pt_cross1']]
    at = 0
    for x, (W, c) in zip(raw, maps):
        assert W.shape == (x.shape[-1], int(g['n_comp'])) and c.shape == (int(g['n_comp']),)
        err = np.abs(x.astype(np.float64) @ W + c - rows[at:at + len(x)]).max()
        print('feature map: max abs err', err, 'bound', bound)
        assert err <= bound
        at += len(x)
    assert at == ntr + len(g['pt_cross0']) + len(g['pt_cross1'])


# ---- end to end ----------------------------------------------------------------------------------------------------------------
def make_three_patients(seed=0, sizes=(128, 96, 96), chans=(8, 10, 12), T=130, ncls=6, latent=6):
    """The task of test_ctc_model_trains_with_the_trainer (three 30-sample segments carrying phoneme patterns in noise),
    in a shared latent space that every patient sees through its own random mixing matrix."""
    rng = np.random.default_rng(seed)
    proto = rng.standard_normal((ncls, latent)).astype(np.float32) * 1.5
    data, labels = [], []
    for n, c in zip(sizes, chans):
        targets = rng.integers(1, ncls, (n, 3))
        z = rng.standard_normal((n, T, latent)).astype(np.float32) * 0.3
        for i in range(n):
            for j in range(3):
                z[i, 20 + 30 * j: 50 + 30 * j] += proto[targets[i, j]]
        mix = rng.standard_normal((latent, c)).astype(np.float32) / np.sqrt(latent)
        data.append((z @ mix + 0.05 * rng.standard_normal((n, T, c)).astype(np.float32)).astype(np.float32))
        labels.append(targets.astype(np.int64))
    return data, labels


def test_cross_patient_ctc_training_end_to_end(tmp_path):
    """Three synthetic patients with different channel counts -> CTCHeldOutTargetValAlignDataModule (PCA, CCA, two
    augmentations, device batches) -> RealtimeRNNModel under the HIP Trainer; the assertions of
    test_ctc_model_trains_with_the_trainer on the held-out target trials.  Learnable at this size: the CPU restatement
    (oracle.realtime_oracle.RealtimeOracle + torch's CTCLoss / AdamW on the same three patients pooled with
    oracle.align_oracle's PCA and CCA, same copies, 200 full-batch epochs) goes from val loss 11.6 / PER 78.6 to 0.16 / 8.3."""
    A = _aug()
    from cross_patient_speech_decoding_amd.nn_models.trainer import Trainer, seed_everything
    from cross_patient_speech_decoding_amd.realtime_sim import CTCHeldOutTargetValAlignDataModule, RealtimeRNNModel
    seed_everything(0)
    (a, b, c), (la, lb, lc) = make_three_patients()
    dm = CTCHeldOutTargetValAlignDataModule(a[:112], la[:112], [b, c], [lb, lc], a[112:], la[112:], batch_size=-1, val_size=0.25,
                                            augmentations=[A.time_shifting, A.scaling], data_path=tmp_path, n_comp=6)
    dm.setup()
    n, T, d = dm.get_data_shape()
    assert (n, T, d) == (3 * (84 + 96 + 96), 130, 6)
    ncls = 6
    model = RealtimeRNNModel(14 * d, 48, 2, ncls, dropout=0.1, learning_rate=1e-2, decay_steps=250)
    tr = Trainer(max_epochs=200, gradient_clip_val=1.0)
    model.cuda()
    before = tr.validate(model, dm.val_dataloader())[0]
    tr.fit(model, dm.train_dataloader(), dm.val_dataloader())
    after = tr.logged_metrics
    print('before', before, 'after', {k: float(v) for k, v in after.items()})
    assert after['train_loss'] < 0.5 * before['val_loss']
    assert after['val_PER'] < 0.5 * before['val_PER'] and after['val_PER'] < 40.0
