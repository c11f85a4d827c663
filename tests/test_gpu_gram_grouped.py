"""gram_grouped_kernel (csrc/xps_fold_align.hip) on the MI355X through the C ABI (xps_gram_grouped_f64), its wrapper
alignment/_linalg.py: gram_grouped, and fit_folds with the held-out rows appended.

References (tests/f64_ref.py): integer-valued operands, for which every summation order gives the same bits (bit-equal to
``exact_product(V, V.T)``), and standard-normal operands against the long-double product within the derived bound
(D + 2) 2^-53 |V| |V^T|.  Conventions: operands live in buffers whose rows are longer than the matrix (ldv = D + 3) with NaN in the
padding; outputs lie between guard rows (tests/guarded_buf.py) and start as a sentinel everywhere, ldg = n + 3, so an element never
written, a padding element written and a guard element written all show."""
import sys

import numpy as np
import pytest

import f64_ref as R
from guarded_buf import SENT64, Buf64

pytestmark = pytest.mark.gpu
needs_long_double = pytest.mark.skipif(not R.have_long_double(), reason=R.LONG_DOUBLE_REASON)

PAD = 3
WORDS = 8
NS, DS = (1, 63, 64, 65, 130), (1, 15, 16, 17, 100)


def torch_():
    import torch
    return torch


def LA():
    from cross_patient_speech_decoding_amd.alignment import _linalg
    return _linalg


def lib():
    from cross_patient_speech_decoding_amd._lib import lib as _l
    return _l()


def dev(a):
    return torch_().from_numpy(np.ascontiguousarray(a)).to(LA().device())


def entry(tab, n_problems, tiles, n_tiles, ws=None, ws_bytes=None):
    """xps_gram_grouped_f64 on host tables (None: a null pointer), then a synchronise."""
    torch = torch_()
    from cross_patient_speech_decoding_amd import _dev
    from cross_patient_speech_decoding_amd._lib import call
    if ws is None:
        ws_bytes = int(lib().xps_gram_grouped_f64_workspace(max(n_problems, 0), max(n_tiles, 0)))
        ws = torch.empty(ws_bytes // 8 + 1, dtype=torch.int64, device=LA().device())
    call('xps_gram_grouped_f64', None if tab is None else tab.ctypes.data, n_problems, None if tiles is None else tiles.ctypes.data,
         n_tiles, ws if isinstance(ws, int) else ws.data_ptr(), ws_bytes, _dev.stream())
    torch.cuda.synchronize()


class Problem:
    """One problem of a launch: V (n x D, `dtype`) in a NaN-padded device buffer, G in a guarded sentinel buffer."""

    def __init__(self, V):
        self.V = V
        self.n, self.D = V.shape
        self.Vd = dev(R.padded(V, PAD, np.nan))
        self.ldg = self.n + PAD
        self.out = Buf64(max(self.n, 1) * self.ldg)

    def row(self):
        return [self.Vd.data_ptr(), int(self.V.dtype == np.float32), self.D + PAD, self.n, self.D, self.out.ptr, self.ldg, 0]

    def result(self):
        """The n x n block as float64; the padding columns and the guards must still hold the sentinel."""
        assert self.out.guards_intact(), 'a guard element was written'
        bits = self.out.numpy((max(self.n, 1), self.ldg))
        assert (bits[:self.n, self.n:] == SENT64).all() and (bits[self.n:] == SENT64).all(), 'padding was written'
        return np.ascontiguousarray(bits[:self.n, :self.n]).view(np.float64)


def launch(problems):
    tab = np.array([p.row() for p in problems], dtype=np.int64).reshape(-1)
    tiles = LA().gram_tiles([p.n for p in problems])
    entry(tab, len(problems), tiles, len(tiles))


def bits(a):
    return np.ascontiguousarray(a).view(np.int64)


# ------------------------------------------------------------------------------------------------ shapes and exactness
@pytest.mark.parametrize('D', DS)
@pytest.mark.parametrize('n', NS)
def test_integer_operands_are_bit_equal_to_the_exact_product(n, D):
    rng = np.random.default_rng(1000 * n + D)
    for dtype in (np.float64, np.float32):
        V = R.int_matrix(rng, (n, D), dtype)
        p = Problem(V)
        launch([p])
        G = p.result()
        np.testing.assert_array_equal(G, R.exact_product(V.astype(np.float64), V.astype(np.float64).T))
        assert np.array_equal(bits(G), bits(G.T))


@needs_long_double
@pytest.mark.parametrize('D', DS)
@pytest.mark.parametrize('n', NS)
def test_real_operands_stay_within_the_derived_bound_and_are_symmetric_and_reproducible(n, D):
    rng = np.random.default_rng(2000 * n + D)
    for dtype in (np.float64, np.float32):
        V = R.real_matrix(rng, (n, D), dtype)
        V64 = V.astype(np.float64)                                 # float32 widens exactly
        a, b = Problem(V), Problem(V)
        launch([a])
        launch([b])
        G = a.result()
        used = R.assert_within(G, R.long_product(V64, V64.T), R.dot_bound(V64, V64.T), f'n={n} D={D} {np.dtype(dtype).name}')
        print(f'n={n} D={D} {np.dtype(dtype).name}: largest error / bound {used:.3f}')
        assert np.array_equal(bits(G), bits(G.T)), 'G is not symmetric bit for bit'
        assert np.array_equal(bits(G), bits(b.result())), 'two launches differ'


def test_one_launch_mixes_shapes_and_types_and_an_empty_problem_writes_nothing():
    rng = np.random.default_rng(7)
    specs = [(130, 100, np.float32, True), (1, 1, np.float64, False), (63, 17, np.float64, True), (65, 16, np.float32, False),
             (0, 10, np.float64, False), (64, 15, np.float64, False)]
    probs = [Problem((R.real_matrix if real else R.int_matrix)(rng, (n, D), dt)) for n, D, dt, real in specs]
    launch(probs)
    alone = [Problem(p.V) for p in probs]
    for p, q, (n, D, dt, real) in zip(probs, alone, specs):
        G = p.result()
        if n == 0:
            assert p.out.untouched()
            continue
        launch([q])
        assert np.array_equal(bits(G), bits(q.result())), 'a problem depends on the table it is in'   # the same for any grid
        assert np.array_equal(bits(G), bits(G.T))
        V64 = p.V.astype(np.float64)
        if real:
            assert np.abs(G - V64 @ V64.T).max() <= 1e-12 * np.abs(G).max()
        else:
            np.testing.assert_array_equal(G, R.exact_product(V64, V64.T))


def test_an_empty_contraction_gives_zeros():
    p = Problem(np.zeros((65, 0)))
    launch([p])
    assert not p.result().any()


# ------------------------------------------------------------------------------------------------ refusals of the entry
def test_the_entry_refuses_bad_tables_before_any_launch():
    from cross_patient_speech_decoding_amd._lib import XpsError
    p, q = Problem(np.ones((70, 5))), Problem(np.ones((0, 5)))
    good = np.array([p.row(), q.row()], dtype=np.int64)
    tiles = LA().gram_tiles([70, 0])
    assert tiles.tolist() == [[0, 0, 0], [0, 1, 0], [0, 1, 1]]

    def refused(match, tab=good, n_problems=2, tl=tiles, n_tiles=None, **kw):
        with pytest.raises(XpsError, match=match):
            entry(None if tab is None else np.ascontiguousarray(tab).reshape(-1), n_problems,
                  None if tl is None else np.ascontiguousarray(tl, dtype=np.int32).reshape(-1), len(tiles) if n_tiles is None else n_tiles, **kw)

    def changed(word, value, prob=0):
        tab = good.copy()
        tab[prob, word] = value
        return tab
    refused('null table', tab=None)
    refused('null table', tl=None)
    refused('negative count', n_problems=-1)
    refused('negative count', n_tiles=-1)
    refused('negative count', tab=changed(3, -1))                 # n
    refused('negative count', tab=changed(4, -1))                 # D
    refused('ldv < D', tab=changed(2, 4))
    refused('ldg < n', tab=changed(6, 69))
    refused('null matrix', tab=changed(0, 0))
    refused('null matrix', tab=changed(5, 0))
    refused('v_is_f32', tab=changed(1, 2))
    refused('names no problem', tl=[[2, 0, 0]], n_tiles=1)
    refused('names no problem', tl=[[-1, 0, 0]], n_tiles=1)
    refused('names no problem', tab=good, n_problems=0, tl=[[0, 0, 0]], n_tiles=1)
    refused('at or past n', tl=[[0, 2, 0]], n_tiles=1)            # 128 >= 70
    refused('at or past n', tl=[[1, 0, 0]], n_tiles=1)            # the empty problem has no tile
    refused('above the diagonal', tl=[[0, 0, 1]], n_tiles=1)
    refused('above the diagonal', tl=[[0, 1, -1]], n_tiles=1)
    refused('null workspace', ws=0, ws_bytes=1 << 20)
    refused('workspace too small', ws=torch_().empty(64, dtype=torch_().int64, device=LA().device()), ws_bytes=8)
    assert p.out.untouched() and q.out.untouched()                # nothing was launched
    entry(good.reshape(-1), 2, tiles, len(tiles))                 # and the table itself is fine
    np.testing.assert_array_equal(p.result(), np.full((70, 70), 5.0))
    entry(None, 0, None, 0)                                       # nothing to do: XPS_OK


def test_gram_grouped_refuses_bad_tensors_before_any_launch(monkeypatch):
    torch, la = torch_(), LA()
    calls = []
    monkeypatch.setattr(la, 'call', lambda name, *a: calls.append(name))
    V = torch.ones(70, 5, dtype=torch.float32, device=la.device())
    G = torch.zeros(70, 70, dtype=torch.float64, device=la.device())
    bad = [(V.cpu(), G), (V, G.cpu()), (V, G.float()), (V, G[:69]), (V, G[:, :69]), (V.t(), torch.zeros(5, 5, dtype=torch.float64, device=la.device())),
           (V.half(), G), (V[0], G), (V, G.t()[::2].t())]
    for Vb, Gb in bad:
        with pytest.raises(ValueError, match='gram_grouped'):
            la.gram_grouped([(V, G), (Vb, Gb)])
    assert calls == [] and not G.any().item()
    assert la.gram_grouped([]) is None


def test_gram_grouped_takes_slices_of_larger_tensors():
    torch, la = torch_(), LA()
    rng = np.random.default_rng(3)
    wide = R.int_matrix(rng, (90, 40), np.float32)
    big = torch.full((100, 100), -77.125, dtype=torch.float64, device=la.device())
    tables = la.gram_grouped([(dev(wide)[5:75, 2:35], big[10:80, 20:90]), (dev(wide[:3]), big[90:93, 0:3])])  # noqa: F841
    got = big.cpu().numpy()
    sub = wide[5:75, 2:35].astype(np.float64)
    np.testing.assert_array_equal(got[10:80, 20:90], sub @ sub.T)
    np.testing.assert_array_equal(got[90:93, 0:3], wide[:3].astype(np.float64) @ wide[:3].astype(np.float64).T)
    got[10:80, 20:90] = -77.125
    got[90:93, 0:3] = -77.125
    assert (got == -77.125).all()


# ------------------------------------------------------------------------------------------------ fit_folds, held-out rows appended
def _count_calls(monkeypatch):
    from collections import Counter
    from cross_patient_speech_decoding_amd import _lib
    counts, real = Counter(), _lib.call

    def counting(name, *args):
        counts[name] += 1
        return real(name, *args)
    for mod in list(sys.modules.values()):                               # every module that bound `call` by name
        if getattr(mod, '__name__', '').startswith('cross_patient_speech_decoding_amd') and getattr(mod, 'call', None) is real:
            monkeypatch.setattr(mod, 'call', counting)
    return counts


def test_fit_folds_appends_the_held_out_rows_in_the_same_launches(monkeypatch):
    from sklearn.model_selection import KFold
    import cross_patient_speech_decoding_amd.alignment as A
    from cross_patient_speech_decoding_amd.utils.synthetic import make_patient
    torch = torch_()
    pats = [make_patient(p, 48 + 3 * p, T=20, C=c, n_cond=12, k=6, noise=0.5) for p, c in enumerate([24, 20, 17])]
    X, y = pats[0]
    pool = [(x, yy, yy) for x, yy in pats[1:]]
    splits = list(KFold(4, shuffle=True, random_state=0).split(X))
    counts = _count_calls(monkeypatch)
    plain = A.fit_folds(X, y, pool, splits)
    before = dict(counts)
    counts.clear()
    held = A.fit_folds(X, y, pool, splits, append_heldout=True)
    assert dict(counts) == before and before['xps_apply_grouped_f64'] == 2
    with pytest.raises(ValueError, match='append_heldout'):
        plain.pool_with_heldout(0)
    for f, (tr, te) in enumerate(splits):
        whole, idx = held.pool_with_heldout(f)
        n_tr = plain.train_pool(f).shape[0]
        assert np.array_equal(idx, te) and whole.shape[0] == n_tr + len(te) and whole.dtype == torch.float32
        assert whole.is_contiguous() and tuple(whole.shape[1:]) == tuple(plain.train_pool(f).shape[1:])
        assert torch.equal(whole[:n_tr], plain.train_pool(f)) and torch.equal(held.train_pool(f), plain.train_pool(f))
        assert torch.equal(whole[n_tr:], held.project(f, te))
    one = A.fit_folds(X, y, pool, splits, max_bytes=1, append_heldout=True)                # one fold per chunk
    for f in range(len(splits)):
        assert torch.equal(one.pool_with_heldout(f)[0], held.pool_with_heldout(f)[0])
