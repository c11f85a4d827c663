"""Generate tests/golden/ctc_data.npz from the REFERENCE's realtime_sim/augmentations.py and realtime_datamodule.py.
Build container only:  python tests/golden/make_ctc_data_fixtures.py <reference checkout>/aligned_decoding
(or REFERENCE_ALIGNED_DECODING in the environment).

torchvision, lightning and h5py are absent: in-process glue modules supply torchvision.transforms.Resize (imported by the
augmentations module, never called by the five per-trial functions), lightning.LightningDataModule (an empty base class)
and an h5py.File that only RECORDS create_dataset calls.  The glue touches no arithmetic: every stored array is what the
reference's own code computed with torch / numpy / scikit-learn on the CPU.

Contents (float32 unless stated; seeds are stored, every per-trial draw is re-derived by re-seeding and repeating the
reference's generator call):
  aug_*      the five augmentations on one host tensor under torch.manual_seed
  red_*      reduce_to_latent_space (of pt_tgt): a fit, a transform with that PCA, and a fit that keeps <= 5 components (re-fit branch)
  align_*    align_to_target (target = red_fit with pt_tgt_labels) with (N, 3) label sequences
  ho_*       one CTCHeldOutTargetValAlignDataModule.setup() (three patients, two augmentations) under np.random.seed /
             torch.manual_seed, with the split indices recovered by matching trials
  cv_*       fold 0 of CTCHeldOutTargetValAlignCVDataModule.setup() under the same kind of seeds, and the indices of all folds"""
import os
import sys
import tempfile
import types

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
RECORDED = {}


def _glue():
    tv, tvt = types.ModuleType('torchvision'), types.ModuleType('torchvision.transforms')
    tvt.Resize = object
    tv.transforms = tvt
    L = types.ModuleType('lightning')

    class LightningDataModule:
        def __init__(self, *a, **k):
            pass
    L.LightningDataModule = LightningDataModule
    h5 = types.ModuleType('h5py')

    class File:
        def __init__(self, path, mode='r'):
            self.name = os.path.basename(str(path))

        def __enter__(self):
            return self

        def __exit__(self, *a):
            return False

        def create_dataset(self, name, data=None):
            RECORDED.setdefault(self.name, {})[name] = None if data is None else np.array(data.numpy() if torch.is_tensor(data) else data)
    h5.File = File
    sys.modules.update({'torchvision': tv, 'torchvision.transforms': tvt, 'lightning': L, 'h5py': h5})


def _match(rows, pool):
    """index in `pool` of every trial of `rows` (exact match of the raw trials)."""
    idx = []
    for r in rows:
        hit = np.flatnonzero((pool == r).reshape(len(pool), -1).all(axis=1))
        assert len(hit) == 1, 'trial not matched uniquely'
        idx.append(int(hit[0]))
    return np.asarray(idx, dtype=np.int64)


def _patients(rng, T, sizes, chans, seqs, latent=4):
    """Three synthetic patients: a shared latent course per label sequence, mixed into each patient's channels, plus noise."""
    course = rng.standard_normal((len(seqs), T, latent)).astype(np.float32)
    data, labels = [], []
    for n, c in zip(sizes, chans):
        which = rng.integers(0, len(seqs), n)
        which[:len(seqs)] = np.arange(len(seqs))                      # every sequence occurs in every patient
        mix = rng.standard_normal((latent, c)).astype(np.float32)
        x = course[which] @ mix + 0.3 * rng.standard_normal((n, T, c)).astype(np.float32)
        data.append(x.astype(np.float32))
        labels.append(seqs[which].astype(np.int64))
    return data, labels


if __name__ == '__main__':
    ref = sys.argv[1] if len(sys.argv) > 1 else os.environ.get('REFERENCE_ALIGNED_DECODING')
    if not ref or not os.path.isdir(os.path.join(ref, 'realtime_sim')):
        sys.exit('usage: make_ctc_data_fixtures.py <reference checkout>/aligned_decoding')
    _glue()
    sys.path.insert(0, ref)
    import sklearn
    from realtime_sim import augmentations as RA                       # noqa: E402
    from realtime_sim import realtime_datamodule as RD                 # noqa: E402

    out = dict(torch_version=np.array(torch.__version__), numpy_version=np.array(np.__version__),
               sklearn_version=np.array(sklearn.__version__))
    rng = np.random.default_rng(2025)

    # ---- the five augmentations on a host tensor ---------------------------------------------------------------------
    N, T, C = 10, 60, 8
    x = torch.from_numpy(rng.standard_normal((N, T, C)).astype(np.float32))
    out['aug_x'] = x.numpy()
    seeds = dict(warp=11, mask=12, shift=13, jitter=14, scale=15)
    out['aug_seeds'] = np.array([seeds[k] for k in ('warp', 'mask', 'shift', 'jitter', 'scale')])
    for name, fn in (('warp', RA.time_warping), ('mask', RA.time_masking), ('shift', RA.time_shifting),
                     ('jitter', RA.noise_jitter), ('scale', RA.scaling)):
        torch.manual_seed(seeds[name])
        out[f'aug_{name}'] = fn(x).numpy()
    torch.manual_seed(seeds['warp'])
    fac = torch.empty(N).uniform_(0.8, 1.2)
    out['aug_warp_factors'] = fac.numpy()
    out['aug_warp_T2'] = np.array([int(T * fac[i]) for i in range(N)], dtype=np.int64)
    torch.manual_seed(seeds['mask'])
    out['aug_mask_size'] = np.array(int(T * 0.1))
    out['aug_mask_starts'] = torch.randint(0, T - int(T * 0.1) + 1, (N,)).numpy()
    torch.manual_seed(seeds['shift'])
    out['aug_shifts'] = torch.randint(-20, 21, (N,)).numpy()
    torch.manual_seed(seeds['jitter'])
    out['aug_jitter_noise'] = torch.randn_like(x).numpy()
    torch.manual_seed(seeds['scale'])
    out['aug_scales'] = torch.empty(N, 1, 1).uniform_(0.9, 1.1).numpy().reshape(-1)

    # ---- reduce_to_latent_space ------------------------------------------------------------------------------------------
    seqs = np.array([[1, 2, 3], [2, 4, 1], [5, 1, 1], [3, 3, 6], [6, 5, 2], [4, 6, 7]])
    (a, b, c3), (la, lb, lc) = _patients(rng, T, (16, 12, 10), (12, 10, 8), seqs)
    red_fit, pca = RD.reduce_to_latent_space(torch.Tensor(a), n_components=6)
    red_tr, _ = RD.reduce_to_latent_space(torch.Tensor(a[:4] * 0.5 + 0.1), pca=pca)
    out.update(red_fit=red_fit.numpy(), red_components=pca.components_, red_mean=pca.mean_,
               red_x2=(a[:4] * 0.5 + 0.1).astype(np.float32), red_transform=red_tr.numpy())
    wide = (rng.standard_normal((6, 20, 4)).astype(np.float32) @ rng.standard_normal((4, 32)).astype(np.float32)
            + 0.2 * rng.standard_normal((6, 20, 32)).astype(np.float32)).astype(np.float32)
    red_re, pca_re = RD.reduce_to_latent_space(torch.Tensor(wide), n_components=4)          # 4 <= low_thresh: re-fit with 30
    assert pca_re.n_components_ == 30
    out.update(red_wide=wide, red_refit=red_re.numpy(), red_refit_components=pca_re.components_)

    # ---- align_to_target with (N, 3) label sequences -------------------------------------------------------------------------
    src, _ = RD.reduce_to_latent_space(torch.Tensor(b), n_components=6)
    al = RD.align_to_target(RD.AlignCCA, red_fit, src, torch.from_numpy(la), torch.from_numpy(lb))
    out.update(align_src=src.numpy(), align_src_labels=lb, align_out=al.numpy())

    # ---- one full CTCHeldOutTargetValAlignDataModule.setup() ----------------------------------------------------------------------
    test = (a[:5] * 0.9).astype(np.float32)
    test_lab = la[:5]
    out.update(pt_tgt=a, pt_tgt_labels=la, pt_cross0=b, pt_cross0_labels=lb, pt_cross1=c3, pt_cross1_labels=lc, pt_test=test,
               pt_test_labels=test_lab, n_comp=np.array(6), val_size=np.array(0.25), ho_seeds=np.array([5, 6]),
               cv_seeds=np.array([7, 8]), cv_folds=np.array(3))
    tmp = tempfile.mkdtemp()
    augs = [RA.time_shifting, RA.scaling]

    def run(cls, seeds, raw=False, **kw):
        RECORDED.clear()
        np.random.seed(int(seeds[0]))
        torch.manual_seed(int(seeds[1]))
        if raw:          # same split draws (the split is the first consumer of numpy's generator), data left as it is
            dm = cls(a, la, None, None, test, test_lab, augmentations=None, data_path=tmp, pool=False, align=False, **kw)
        else:
            dm = cls(a, la, [b, c3], [lb, lc], test, test_lab, augmentations=augs, data_path=tmp, pool=True, n_comp=6,
                     align=True, **kw)
        dm.setup()
        return {k: dict(v) for k, v in RECORDED.items()}

    rec = run(RD.CTCHeldOutTargetValAlignDataModule, out['ho_seeds'], val_size=0.25)['rnn_realtime.h5']
    raw = run(RD.CTCHeldOutTargetValAlignDataModule, out['ho_seeds'], raw=True, val_size=0.25)['rnn_realtime.h5']
    out['ho_train_idx'], out['ho_val_idx'] = _match(raw['train_data'], a), _match(raw['val_data'], a)
    assert np.array_equal(raw['val_labels'], rec['val_labels'])
    for k, v in rec.items():
        out[f'ho_{k}'] = v

    recs = run(RD.CTCHeldOutTargetValAlignCVDataModule, out['cv_seeds'], n_folds=3)
    raws = run(RD.CTCHeldOutTargetValAlignCVDataModule, out['cv_seeds'], raw=True, n_folds=3)
    for f in range(3):
        r = raws[f'rnn_realtime_fold{f}.h5']
        out[f'cv_train_idx{f}'], out[f'cv_val_idx{f}'] = _match(r['train_data'], a), _match(r['val_data'], a)
        assert np.array_equal(r['val_labels'], recs[f'rnn_realtime_fold{f}.h5']['val_labels'])
    for k, v in recs['rnn_realtime_fold0.h5'].items():
        out[f'cv_{k}'] = v

    path = os.path.join(HERE, 'ctc_data.npz')
    np.savez_compressed(path, **out)
    print('ctc_data.npz', os.path.getsize(path), 'bytes;', {k: v.shape for k, v in out.items() if k.startswith(('ho_', 'cv_'))})
