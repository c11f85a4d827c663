"""Data modules of cross-patient CTC training -- counterpart of the reference's realtime_sim/realtime_datamodule.py
(CTCHeldOutDataModule :23, CTCHeldOutTargetValDataModule :176, CTCHeldOutTargetValAlignDataModule :257,
CTCHeldOutTargetValCVDataModule :404, CTCHeldOutTargetValAlignCVDataModule :578, CTCDataset :727, select_cv :787,
reduce_to_latent_space :813, align_to_target :872).  Same names, constructor arguments and methods (setup / set_fold /
train|val|test_dataloader / get_data_shape).

The five modules differ only in where the validation split comes from (a held-out fraction or k folds, always of the TARGET
patient) and in what happens to the cross patients (none, appended as given, or PCA-reduced and CCA-aligned per split), so
they share one base.  By design:
  * PCA is alignment.pca.PCA and the aligner defaults to the package's AlignCCA: both fit on the MI355X;
  * every stage rounds to float32 where the reference's ``torch.Tensor(...)`` casts do (after each PCA, after the alignment);
  * the pooled training tensor is allocated once on the device and every piece -- target rows, aligned cross-patient rows,
    one augmented copy per augmentation -- is written into its slab (no torch.cat copies); the loaders yield device batches
    (x, y, input_lengths, target_lengths), the 4-tuples ``RealtimeRNNModel`` trains on;
  * split caches live in memory, and with ``save_folds=True`` as ``rnn_realtime.npz`` / ``rnn_realtime_fold{k}.npz`` under
    ``data_path`` with the reference's dataset names (h5py is not available); ``load_folds()`` reads them back;
  * ``reduce_to_latent_space`` follows the reference's code, not its comment: when the first fit keeps
    ``n_components_ <= low_thresh`` components it re-fits with 30 and drops nothing;
  * like the reference, ``dim_red`` is stored and not used (its setup always reduces with PCA).

Extensions (keyword-only): ``split_indices`` pins the otherwise unseeded split -- (train_idx, val_idx) for the held-out
modules, a list of such pairs (one per fold) for the CV modules -- and ``feature_maps()`` returns, after ``setup()``, the
affine map (W, c) of every patient from raw channels to the pooled space (target: its PCA; cross patient j: its PCA, then
its AlignCCA 'b_to_a'): the values ``RealtimePipeline(feature_map=...)`` takes."""
import os
from pathlib import Path

import numpy as np
import torch
from sklearn.model_selection import KFold, StratifiedKFold, train_test_split

from .._dev import current_device
from ..alignment import PCA, AlignCCA
from .realtime_pipeline import feature_map_from

FOLD_KEYS = ('train_data', 'train_labels', 'val_data', 'val_labels', 'test_data', 'test_labels')
_WHO = 'cross_patient_speech_decoding_amd: CTC data module setup'        # named by the "needs the MI355X" error


def _f32(x):
    """torch.Tensor(x): a float32 host tensor (a tensor keeps its device)."""
    return x.detach().float() if torch.is_tensor(x) else torch.Tensor(np.asarray(x))


def _long(x):
    return (x.detach() if torch.is_tensor(x) else torch.as_tensor(np.asarray(x))).long()


def _np(x):
    return x.detach().cpu().numpy() if torch.is_tensor(x) else np.asarray(x)


class CTCDataset(torch.utils.data.Dataset):
    """(features, labels, input_length, target_length) items for the CTC loss (reference :727-754)."""

    def __init__(self, X, y):
        self.X = X
        self.y = y

    def __len__(self):
        return len(self.X)

    def __getitem__(self, idx):
        return self.X[idx], self.y[idx], len(self.X[idx]), len(self.y[idx])


class _BatchLoader:
    """The DataLoader(CTCDataset(X, y), batch_size, shuffle) of the reference over tensors that already live on the device:
    a batch is four device tensors (X[idx], y[idx], input_lengths, target_lengths), gathered by one index per batch."""

    def __init__(self, dataset, batch_size, shuffle):
        self.dataset, self.batch_size, self.shuffle = dataset, int(batch_size), shuffle

    def __len__(self):
        return (len(self.dataset) + self.batch_size - 1) // self.batch_size if len(self.dataset) else 0

    def __iter__(self):
        X, y = self.dataset.X, self.dataset.y
        n = len(X)
        order = torch.randperm(n).to(X.device) if self.shuffle else None
        for s in range(0, n, self.batch_size):
            if order is None:
                xb, yb = X[s:s + self.batch_size], y[s:s + self.batch_size]
            else:
                idx = order[s:s + self.batch_size]
                xb, yb = X[idx], y[idx]
            nb = xb.shape[0]
            yield (xb, yb, torch.full((nb,), X.shape[1], dtype=torch.int64, device=X.device),
                   torch.full((nb,), y.shape[1], dtype=torch.int64, device=X.device))


def select_cv(folds, labels):
    """StratifiedKFold when every class (of the first label column) has at least ``folds`` trials, else KFold (:787-810)."""
    labels = torch.as_tensor(labels)
    cv_labels = labels[:, 0] if len(labels.shape) > 1 else labels
    class_counts = torch.bincount(cv_labels)
    if (class_counts < folds).any():
        return KFold(n_splits=folds, shuffle=True)
    return StratifiedKFold(n_splits=folds, shuffle=True)


def reduce_to_latent_space(data, pca=None, n_components=30, low_thresh=5):
    """(N, T, C) tensor -> ((N, T, k) float32 tensor, fitted PCA) (:813-869).  ``pca`` given: transform only.  Otherwise fit
    alignment.pca.PCA(n_components); when that keeps ``n_components_ <= low_thresh`` components, re-fit with 30 (nothing is
    dropped: the reference's code).  Computed on the device in float64 and rounded to float32 once; a device tensor in
    gives a device tensor out."""
    data = torch.as_tensor(data)
    shapes = data.shape
    host = not data.is_cuda
    data_2d = data.reshape(-1, shapes[-1]).to(current_device(_WHO))
    if pca is not None:
        dr = pca
    else:
        dr = PCA(n_components=n_components).fit(data_2d)
        if dr.n_components_ <= low_thresh:
            dr = PCA(n_components=30).fit(data_2d)
    if hasattr(dr, 'transform_device'):
        data_r = dr.transform_device(data_2d.contiguous() if data_2d.dtype in (torch.float32, torch.float64)
                                     else data_2d.double().contiguous(), out_f32=True)
    else:                                   # any fitted object with sklearn's transform()
        data_r = torch.Tensor(np.asarray(dr.transform(_np(data_2d)))).to(data_2d.device)
    data_r = data_r.reshape(shapes[0], shapes[1], -1)
    return (data_r.cpu() if host else data_r), dr


def _align_fit(aligner, target_data, source_data, target_labels, source_labels):
    align = aligner()
    align.fit(target_data, source_data, _np(target_labels), _np(source_labels))
    return align


def _align_apply(align, source_data):
    shp = source_data.shape
    source_a = align.transform(source_data)
    source_a = source_a.float() if torch.is_tensor(source_a) else torch.Tensor(np.asarray(source_a))
    return source_a.reshape(shp[0], shp[1], -1)


def align_to_target(aligner, target_data, source_data, target_labels, source_labels):
    """Fit ``aligner()`` on (target, source) with their labels and map the source trials into the target's space
    (:872-894); float32, on the source tensor's device."""
    source_data = torch.as_tensor(source_data)
    out = _align_apply(_align_fit(aligner, target_data, source_data, target_labels, source_labels), source_data)
    return out.to(source_data.device)


class _CTCModule:
    """Shared machinery: split of the target patient, optional PCA / alignment per split, pooling and augmentation into
    one device tensor, the split cache and the loaders.  Subclasses set ``cv`` (k folds instead of a held-out fraction)
    and ``per_patient`` (cross patients as a list, reduced and aligned per split)."""

    cv = False
    per_patient = False

    def _init(self, train_data_tgt, train_labels_tgt, train_data_cross, train_labels_cross, test_data, test_labels,
              batch_size, val_size, n_folds, augmentations, data_path, split_indices, save_folds, pool=False, dim_red=PCA,
              n_comp=30, align=False, aligner=AlignCCA):
        self.train_data_tgt = _f32(train_data_tgt)
        self.train_labels_tgt = _long(train_labels_tgt)
        if train_data_cross is None:
            self.train_data_cross = self.train_labels_cross = None
        elif self.per_patient:
            self.train_data_cross = [_f32(d) for d in train_data_cross]
            self.train_labels_cross = [_long(lab) for lab in train_labels_cross]
        else:
            self.train_data_cross = _f32(train_data_cross)
            self.train_labels_cross = _long(train_labels_cross)
        self.test_data = _f32(test_data)
        self.test_labels = _long(test_labels)
        self.batch_size = batch_size
        self.val_size, self.n_folds = val_size, n_folds
        self.augmentations = augmentations if augmentations else []
        self.current_fold = 0
        self.data_path = Path(os.getcwd() if data_path is None else data_path)
        self.split_indices, self.save_folds = split_indices, save_folds
        self.pool, self.dim_red, self.n_components, self.align, self.aligner = pool, dim_red, n_comp, align, aligner
        self._folds, self._maps = {}, {}

    # ---- the split of the target patient --------------------------------------------------------------------------
    def _splits(self):
        """[(train_idx, val_idx or None)] over the target patient's trials; one entry per fold (held-out: one)."""
        n = len(self.train_data_tgt)
        labels = self.train_labels_tgt
        if self.split_indices is not None:
            pairs = self.split_indices if self.cv else [self.split_indices]
            if self.cv and len(pairs) != self.n_folds:
                raise ValueError(f'{len(pairs)} split_indices pairs for {self.n_folds} folds')
            return [(np.asarray(tr, dtype=np.int64), None if va is None else np.asarray(va, dtype=np.int64)) for tr, va in pairs]
        if self.cv:
            return [(tr, va) for tr, va in select_cv(self.n_folds, labels).split(np.zeros(n), _np(labels))]   # the reference's draws
        if not self.val_size > 0:
            return [(np.arange(n), None)]
        n_classes = len(torch.unique(labels))
        if self.val_size * n < n_classes:
            split_labels = None
        elif len(labels.shape) > 1:
            split_labels = _np(labels[:, 0])
        else:
            split_labels = _np(labels)
        tr, va = train_test_split(np.arange(n), test_size=self.val_size, stratify=split_labels)   # the reference's draws
        return [(tr, va)]

    # ---- one split: reduce, align, pool, augment -------------------------------------------------------------------
    def _build(self, key, tr, va):
        dev = current_device(_WHO)
        take = lambda t, i: t[torch.as_tensor(i, dtype=torch.int64)]                          # noqa: E731
        tgt, tgt_lab = take(self.train_data_tgt, tr).to(dev), take(self.train_labels_tgt, tr)
        val = None if va is None else take(self.train_data_tgt, va).to(dev)
        val_lab = None if va is None else take(self.train_labels_tgt, va)
        test, test_lab = self.test_data.to(dev), self.test_labels
        if self.train_data_cross is None:
            cross, cross_lab = [], []
        elif self.per_patient:
            cross, cross_lab = [d.to(dev) for d in self.train_data_cross], list(self.train_labels_cross)
        else:
            cross, cross_lab = [self.train_data_cross.to(dev)], [self.train_labels_cross]
        maps = None
        if self.per_patient and self.pool:
            tgt, tgt_pca = reduce_to_latent_space(tgt, n_components=self.n_components)
            if val is not None:
                val, _ = reduce_to_latent_space(val, pca=tgt_pca)
            test, _ = reduce_to_latent_space(test, pca=tgt_pca)
            pcas = []
            for j in range(len(cross)):
                cross[j], p = reduce_to_latent_space(cross[j], n_components=self.n_components)
                pcas.append(p)
            if self.align:
                aligners = []
                for j in range(len(cross)):
                    al = _align_fit(self.aligner, tgt, cross[j], tgt_lab, cross_lab[j])
                    cross[j] = _align_apply(al, cross[j])
                    aligners.append(al)
                maps = [(tgt_pca,)] + [(p, al) for p, al in zip(pcas, aligners)]
            else:
                min_dim = min(d.shape[-1] for d in [tgt] + cross)
                tgt, test = tgt[:, :, :min_dim], test[:, :, :min_dim]
                val = None if val is None else val[:, :, :min_dim]
                cross = [d[:, :, :min_dim] for d in cross]
                maps = [(tgt_pca,)] + [(p,) for p in pcas]
                maps = [m + (min_dim,) for m in maps]
        self._maps[key] = maps

        # pooled rows: target, then the cross patients, then one augmented copy of all of them per augmentation
        parts = [tgt] + cross
        n_pool = sum(len(p) for p in parts)
        copies = 1 + len(self.augmentations)
        train = torch.empty((copies * n_pool,) + tuple(tgt.shape[1:]), dtype=torch.float32, device=dev)
        at = 0
        for p in parts:
            train[at:at + len(p)].copy_(p)
            at += len(p)
        pooled = train[:n_pool]
        for a, aug in enumerate(self.augmentations, 1):
            slab = train[a * n_pool:(a + 1) * n_pool]
            if getattr(getattr(aug, 'func', aug), 'writes_out', False):
                aug(pooled, out=slab, draw_device='cpu')        # the reference augments host tensors: CPU generator
            else:
                slab.copy_(torch.as_tensor(aug(pooled)).to(dev))
        labels = torch.cat([tgt_lab] + cross_lab)
        labels = torch.cat([labels] * copies)
        self._store(key, train_data=train, train_labels=labels, val_data=val, val_labels=val_lab, test_data=test.contiguous(),
                    test_labels=test_lab)

    def setup(self, stage=None):
        for key, (tr, va) in enumerate(self._splits()):
            self._build(key, tr, va)

    # ---- cache and loaders -------------------------------------------------------------------------------------------
    def _file(self, key):
        return self.data_path / (f'rnn_realtime_fold{key}.npz' if self.cv else 'rnn_realtime.npz')

    def _store(self, key, **arrays):
        dev = current_device(_WHO)
        self._folds[key] = {n: (None if a is None else a.to(dev).contiguous()) for n, a in arrays.items()}
        if self.save_folds:
            os.makedirs(self.data_path, exist_ok=True)
            np.savez(self._file(key), **{n: _np(a) for n, a in arrays.items() if a is not None})

    def load_folds(self):
        """Re-populate the cache from the ``.npz`` files ``save_folds=True`` wrote (a missing validation split stays None)."""
        dev = current_device(_WHO)
        for key in range(self.n_folds if self.cv else 1):
            with np.load(self._file(key)) as f:
                self._folds[key] = {n: (torch.as_tensor(f[n]).to(dev) if n in f.files else None) for n in FOLD_KEYS}
        return self

    def _loader(self, which, shuffle):
        f = self._folds[self.current_fold]
        d, l = f[f'{which}_data'], f[f'{which}_labels']
        if d is None:
            return None
        if l.dim() == 1:
            l = l.reshape(-1, 1)
        n = len(d) if self.batch_size == -1 else self.batch_size
        return _BatchLoader(CTCDataset(d, l), max(n, 1), shuffle)

    def train_dataloader(self):
        return self._loader('train', True)

    def val_dataloader(self):
        return self._loader('val', False)

    def test_dataloader(self):
        return self._loader('test', False)

    def get_data_shape(self):
        return tuple(self._folds[self.current_fold]['train_data'].shape)

    def set_fold(self, fold):
        assert 0 <= fold < (self.n_folds if self.cv else 1), "Fold index out of range"
        self.current_fold = fold

    def feature_maps(self):
        """[(W, c)] of the current split, target first then every cross patient: x_raw @ W + c = that patient's rows of the
        pooled space (feature_map_from over its PCA and, when aligned, its AlignCCA).  Needs ``pool=True``."""
        maps = self._maps.get(self.current_fold)
        if maps is None:
            raise RuntimeError('feature_maps() needs setup() of a module that pools (pool=True)')
        out = []
        for m in maps:
            cut = m[-1] if isinstance(m[-1], int) else None
            W, c = feature_map_from(*(m[:-1] if cut is not None else m))
            out.append((W[:, :cut], c[:cut]) if cut is not None else (W, c))
        return out


class CTCHeldOutDataModule(_CTCModule):
    """One patient, held-out validation fraction (reference :23-173)."""

    def __init__(self, train_data, train_labels, test_data, test_labels, batch_size=128, val_size=0.2, augmentations=None,
                 data_path=None, *, split_indices=None, save_folds=False):
        self._init(train_data, train_labels, None, None, test_data, test_labels, batch_size, val_size, 1, augmentations,
                   data_path, split_indices, save_folds)

    @property
    def train_data(self):
        return self.train_data_tgt

    @property
    def train_labels(self):
        return self.train_labels_tgt


class CTCHeldOutTargetValDataModule(_CTCModule):
    """Validation fraction of the target patient; pre-concatenated cross-patient trials join the training rows (:176-254)."""

    def __init__(self, train_data_tgt, train_labels_tgt, train_data_cross, train_labels_cross, test_data, test_labels,
                 batch_size=128, val_size=0.2, augmentations=None, data_path=None, *, split_indices=None, save_folds=False):
        self._init(train_data_tgt, train_labels_tgt, train_data_cross, train_labels_cross, test_data, test_labels, batch_size,
                   val_size, 1, augmentations, data_path, split_indices, save_folds)


class CTCHeldOutTargetValAlignDataModule(_CTCModule):
    """Validation fraction of the target patient; every cross patient (a list) is PCA-reduced and aligned to the target's
    training rows (:257-401): the module scripts/train_ctc_rnn.py of the reference trains on."""

    per_patient = True

    def __init__(self, train_data_tgt, train_labels_tgt, train_data_cross, train_labels_cross, test_data, test_labels,
                 batch_size=128, val_size=0.2, augmentations=None, data_path=None, pool=True, dim_red=PCA, n_comp=30,
                 align=True, aligner=AlignCCA, *, split_indices=None, save_folds=False):
        self._init(train_data_tgt, train_labels_tgt, train_data_cross, train_labels_cross, test_data, test_labels, batch_size,
                   val_size, 1, augmentations, data_path, split_indices, save_folds, pool, dim_red, n_comp, align, aligner)


class CTCHeldOutTargetValCVDataModule(_CTCModule):
    """k validation folds of the target patient; pre-concatenated cross-patient trials join every fold (:404-575)."""

    cv = True

    def __init__(self, train_data_tgt, train_labels_tgt, train_data_cross, train_labels_cross, test_data, test_labels,
                 batch_size=128, n_folds=5, augmentations=None, data_path=None, *, split_indices=None, save_folds=False):
        self._init(train_data_tgt, train_labels_tgt, train_data_cross, train_labels_cross, test_data, test_labels, batch_size,
                   None, n_folds, augmentations, data_path, split_indices, save_folds)


class CTCHeldOutTargetValAlignCVDataModule(_CTCModule):
    """k validation folds of the target patient; PCA and alignment are learned per fold on its training rows (:578-724)."""

    cv = True
    per_patient = True

    def __init__(self, train_data_tgt, train_labels_tgt, train_data_cross, train_labels_cross, test_data, test_labels,
                 batch_size=128, n_folds=5, augmentations=None, data_path=None, pool=True, dim_red=PCA, n_comp=30,
                 align=True, aligner=AlignCCA, *, split_indices=None, save_folds=False):
        self._init(train_data_tgt, train_labels_tgt, train_data_cross, train_labels_cross, test_data, test_labels, batch_size,
                   None, n_folds, augmentations, data_path, split_indices, save_folds, pool, dim_red, n_comp, align, aligner)
