"""The exact t-SNE kernels of csrc/xps_tsne.hip on the MI355X through the C ABI (xps_tsne_sqdist_f32, xps_tsne_affinities_f64,
xps_tsne_descent_f64), held to the restatement of tests/tsne_ref.py within bars derived from each case's data; every output lies
between guard rows (tests/guarded_buf.py) and every workspace has its exact size.

Each layer is held on the layer below as the DEVICE made it: the search on the device's own d2, the objective and the
trajectories on the device's own P.  Why these launches are in bounds (read in csrc/xps_tsne.hip before they ran): every kernel
indexes rows below n and columns j < n of n x n matrices, state arrays at HEAD + k n + i with k < 15 and i < n; the entries check
n, n_components, the tile table and the workspace before any launch."""
import numpy as np
import pytest
import torch

import cluster_ref as CR
import tsne_ref as TR
from guarded_buf import Buf, Buf64

pytestmark = pytest.mark.gpu

CASES = TR.cases()
NAMES = sorted(CASES)
U = TR.U
_dev = {}


def LA():
    from cross_patient_speech_decoding_amd.alignment import _linalg
    return _linalg


def LIB():
    from cross_patient_speech_decoding_amd import _lib
    return _lib


def f64(buf):
    return buf.view().view(torch.float64)


def bits(a):
    return np.ascontiguousarray(np.asarray(a, dtype=np.float64)).view(np.int64)


def run(name, probs, *args):
    """One entry through the C ABI with the workspace at its exact size between guards."""
    la, lib = LA(), LIB()
    tab, tiles = la.tsne_table(probs), la.tsne_tiles([p['n'] for p in probs])
    nb = int(getattr(lib.lib(), name + '_workspace')(len(probs), len(tiles)))
    assert nb % 8 == 0 and nb == 8 * 16 * len(probs) + 8 * len(tiles)
    ws = Buf64(nb // 8)
    lib.call(name, tab.ctypes.data, len(probs), tiles.ctypes.data, len(tiles), *args, ws.ptr, nb, la.stream())
    torch.cuda.synchronize()
    assert ws.guards_intact()
    return tab, tiles


def gram(X):
    la = LA()
    Xd = la.to_device(X).reshape(len(X), -1)
    Xc = Xd.to(la.F64) - la.col_mean(Xd)
    G = torch.empty(len(X), len(X), dtype=la.F64, device=Xd.device)
    keep = la.gram_grouped([(Xc, G)])
    torch.cuda.synchronize()
    del keep
    return G


def sqdist_problem(name):
    X, _ = CASES[name]
    n = len(X)
    buf = Buf(n * n)
    return dict(n=n, G=gram(X), D2=buf.view().view(n, n), _bufs=[buf])


def affinity_buffers(n):
    b = dict(C=Buf64(n * n), P=Buf64(n * n), beta=Buf64(n), rowsum=Buf64(n), steps=Buf(n))
    pr = dict(n=n, C=f64(b['C']).view(n, n), P=f64(b['P']).view(n, n), beta=f64(b['beta']), rowsum=f64(b['rowsum']),
              steps=b['steps'].view().view(torch.int32), _bufs=list(b.values()))
    return pr


def device_affinities(name):
    """(d2, C, P, beta, steps, rowsum) of a case as the device makes them, alone in its launch; computed once, left unchanged."""
    if name not in _dev:
        pr = sqdist_problem(name)
        run('xps_tsne_sqdist_f32', [pr])
        d2 = pr['D2'].cpu().numpy().copy()
        ap = affinity_buffers(pr['n'])
        ap['D2'] = pr['D2'].contiguous()
        run('xps_tsne_affinities_f64', [ap], float(CASES[name][1]))
        assert all(b.guards_intact() for b in pr['_bufs'] + ap['_bufs'])
        _dev[name] = dict(d2=d2, **{k: ap[k].cpu().numpy().copy() for k in ('C', 'P', 'beta', 'steps', 'rowsum')})
    return _dev[name]


# ------------------------------------------------------------------------------------------------ step 1
@pytest.mark.parametrize('name', NAMES)
def test_d2_is_the_float32_squared_distance_within_the_gram_bar(name):
    X, _ = CASES[name]
    d2 = device_affinities(name)['d2']
    assert d2.dtype == np.float32 and (np.diag(d2) == 0).all() and (d2 >= 0).all() and np.array_equal(d2, d2.T)
    ref = np.asarray(CR.sq_dists(X), dtype=np.float64)
    bar = TR.sqdist_bar(X)
    err = np.abs(d2.astype(np.float64) - ref)
    print(f'{name}: d2 uses {(err / bar).max():.2e} of its bar')
    assert (err <= bar).all()


def test_d2_of_a_batch_has_the_bits_of_each_problem_alone():
    probs = [sqdist_problem(name) for name in NAMES]
    run('xps_tsne_sqdist_f32', probs)
    for name, pr in zip(NAMES, probs):
        assert pr['_bufs'][0].guards_intact()
        assert np.array_equal(pr['D2'].cpu().numpy().view(np.int32), device_affinities(name)['d2'].view(np.int32)), name


# ------------------------------------------------------------------------------------------------ steps 2 and 3
@pytest.mark.parametrize('name', NAMES)
def test_search_and_joint_probabilities_follow_the_restatement_on_the_devices_own_d2(name):
    dv = device_affinities(name)
    n = len(dv['d2'])
    sr = TR.search(dv['d2'], CASES[name][1])
    ok = ~sr.undecided
    assert sr.undecided.sum() <= 0.02 * n
    assert np.array_equal(dv['steps'][ok], sr.steps[ok]), 'step counts differ on a decided row'
    assert np.array_equal(bits(dv['beta'][ok]), bits(sr.beta[ok])), 'beta differs on a decided row'
    exhausted = ok & (sr.steps == 100)
    assert (dv['steps'][exhausted] == 100).all()
    errC = np.abs(dv['C'] - sr.C)
    assert (errC[ok] <= sr.C_bar[ok]).all(), (errC[ok] / np.where(sr.C_bar[ok] > 0, sr.C_bar[ok], 1)).max()
    assert (np.diag(dv['C']) == 0).all()
    rs_bar = sr.C_bar.sum(axis=1) + TR.sum_bar(n) * np.abs(sr.C).sum(axis=1)
    assert (np.abs(dv['rowsum'] - sr.rowsum)[ok] <= rs_bar[ok]).all()
    P = TR.joint(sr.C, sr.rowsum)
    both = ok[:, None] & ok[None, :]
    pbar = TR.joint_bar(sr)
    errP = np.abs(dv['P'] - P)
    assert (errP[both] <= pbar[both]).all()
    assert np.isfinite(dv['P']).all() and (np.diag(dv['P']) == 0).all() and np.array_equal(bits(dv['P']), bits(dv['P'].T))
    offd = ~np.eye(n, dtype=bool)
    assert (dv['P'][offd] >= TR.EPS).all()
    clamped = offd & ((sr.C + sr.C.T) / (2 * sr.rowsum.sum()) < TR.EPS / 2) & both
    assert (dv['P'][clamped] == TR.EPS).all()
    print(f'{name}: C uses {(errC[ok] / np.where(sr.C_bar[ok] > 0, sr.C_bar[ok], np.inf)).max():.2e} of its bar, P '
          f'{(errP[both] / np.where(pbar[both] > 0, pbar[both], np.inf)).max():.2e}; exhausted rows {int((dv["steps"] == 100).sum())}, undecided {int(sr.undecided.sum())}')


def test_affinities_of_a_batch_have_the_bits_of_each_problem_alone():
    probs = []
    for name in NAMES:
        ap = affinity_buffers(len(CASES[name][0]))
        ap['D2'] = torch.from_numpy(device_affinities(name)['d2']).cuda()
        probs.append(ap)
    by_perp = {}
    for name, ap in zip(NAMES, probs):
        by_perp.setdefault(CASES[name][1], []).append((name, ap))
    for perp, group in by_perp.items():                       # the perplexity is one argument of the call
        run('xps_tsne_affinities_f64', [ap for _, ap in group], float(perp))
        for name, ap in group:
            assert all(b.guards_intact() for b in ap['_bufs'])
            for key in ('C', 'P', 'beta', 'rowsum'):
                assert np.array_equal(bits(ap[key].cpu().numpy()), bits(device_affinities(name)[key])), (name, key)
            assert np.array_equal(ap['steps'].cpu().numpy(), device_affinities(name)['steps'])


# ------------------------------------------------------------------------------------------------ steps 4 - 6
def descent_problem(name, Y0, nc, it_begin, lr):
    la = LA()
    dv = device_affinities(name)
    n = len(dv['P'])
    words = 2 * (la.TSNE_STATE_HEAD + la.TSNE_STATE_ARRAYS * n)
    assert int(LIB().lib().xps_tsne_state_bytes(n)) == 8 * words
    st, yo = Buf64(words), Buf64(n * nc)
    return dict(n=n, nc=nc, P=torch.from_numpy(dv['P']).cuda(), Y_in=torch.from_numpy(np.ascontiguousarray(Y0)).cuda(),
                Y_out=f64(yo).view(n, nc), state=f64(st), it_begin=it_begin, lr=lr, _bufs=[st, yo])


def state_half(pr, h):
    la = LA()
    n = pr['n']
    size = la.TSNE_STATE_HEAD + la.TSNE_STATE_ARRAYS * n
    raw = pr['state'].cpu().numpy()[h * size:(h + 1) * size]
    names = ['Y0', 'Y1', 'U0', 'U1', 'GA0', 'GA1', 'GR0', 'GR1', 's', 'a0', 'a1', 'b0', 'b1', 'e1', 'e2']
    out = {k: raw[8 + i * n:8 + (i + 1) * n] for i, k in enumerate(names)}
    out.update(it=raw[0], error=raw[1], best_error=raw[2], best_it=raw[3], done=raw[4], Z=raw[5], norm=raw[6])
    return out


@pytest.mark.parametrize('nc', [1, 2])
@pytest.mark.parametrize('exag', [12.0, 1.0])
@pytest.mark.parametrize('name', NAMES)
def test_one_launch_gives_the_partial_sums_gradient_and_error_of_the_long_double_twin(name, exag, nc):
    P = device_affinities(name)['P']
    n = len(P)
    Y0 = np.random.default_rng(3).standard_normal((n, nc)) * 2.0
    lr = 50.0
    pr = descent_problem(name, Y0, nc, 0, lr)
    run('xps_tsne_descent_f64', [pr], 1, 1, 0.5, exag, 300, 1e-7)          # max_iter = 1: iteration 0 is the last, so it takes the error
    assert all(b.guards_intact() for b in pr['_bufs'])
    h0, h1 = state_half(pr, 0), state_half(pr, 1)
    ptl = TR.partials(P, Y0, True, TR.LD)
    bars = TR.partials_bars(P, Y0)
    used = {}
    for key, got, ref, bar in (('s', h0['s'], ptl.s, bars['s']), ('e1', h0['e1'], ptl.e1, bars['e1']), ('e2', h0['e2'], ptl.e2, bars['e2']),
                               ('a', np.stack([h0['a0'], h0['a1']], 1), ptl.a, bars['a']),
                               ('b', np.stack([h0['b0'], h0['b1']], 1), ptl.b, bars['b'])):
        err = np.abs(got - np.asarray(ref, np.float64))
        assert (err <= bar).all(), (key, (err / np.where(bar > 0, bar, 1)).max())
        used[key] = float((err / np.where(bar > 0, bar, np.inf)).max())
    pt = TR.partials(P, Y0, True)
    Zl, gl, el = TR.objective(ptl, exag, TR.LD)
    dZ, dg, derr = TR.objective_bars(pt, bars, exag)
    g = np.stack([h1['GR0'], h1['GR1']], 1)
    assert abs(h1['Z'] - float(Zl)) <= dZ
    assert (np.abs(g - np.asarray(gl, np.float64))[:, :nc] <= dg[:, :nc]).all()
    assert abs(h1['error'] - float(el)) <= derr, (h1['error'], float(el), derr)
    assert h1['done'] == 1.0 and h1['it'] == 0.0 and h0['done'] == 0.0 and h0['best_error'] == TR.DBL_MAX
    # the step itself, bit for bit from the device's own gradient: update = 0, so every gain decays to 0.8
    ga = np.stack([h1['GA0'], h1['GA1']], 1)
    up = np.stack([h1['U0'], h1['U1']], 1)
    assert (ga[:, :nc] == 0.8).all() and (ga[:, nc:] == 1.0).all() and (g[:, nc:] == 0).all()
    want_u = 0.5 * np.zeros_like(g) - lr * (g * 0.8)
    assert np.array_equal(bits(up[:, :nc]), bits(want_u[:, :nc]))
    Yout = pr['Y_out'].cpu().numpy()
    assert np.array_equal(bits(Yout), bits(Y0 + want_u[:, :nc]))
    print(f'{name} e={exag} nc={nc}: fractions of the bars used: ' + ', '.join(f'{k} {v:.2e}' for k, v in used.items())
          + f', Z {abs(h1["Z"] - float(Zl)) / dZ:.2e}, error {abs(h1["error"] - float(el)) / derr:.2e}')


@pytest.mark.parametrize('nc', [1, 2])
@pytest.mark.parametrize('name', NAMES)
def test_ten_launches_and_a_phase_reset_follow_the_float64_restatement(name, nc):
    P = device_affinities(name)['P']
    n = len(P)
    lr = max(n / 12.0 / 4.0, 50.0)
    Y0 = TR.random_init(n, nc, 7)
    for plan in ([(0, 10, 0.5, 12.0)], [(0, 5, 0.5, 12.0), (5, 10, 0.8, 1.0)]):
        runs = {}
        for dt in (np.float64, TR.LD):
            traj, Yin, und = [], Y0, []
            for it, max_iter, momentum, exag in plan:
                ph = TR.Descent(P, Yin, nc, it, max_iter, momentum, exag, lr, dtype=dt, track=dt is np.float64).run(max_iter - it)
                traj, Yin, und = traj + ph.trajectory, ph.Y_out, und + ph.undecided
            runs[dt] = traj
            if dt is np.float64:
                assert np.mean([u.mean() for u in und]) == 0.0, 'a gains element of the reference is too close to call'
        bars = TR.trajectory_bars(runs[np.float64], runs[TR.LD])
        Yin, t = Y0, -1
        for it, max_iter, momentum, exag in plan:
            pr = descent_problem(name, Yin, nc, it, lr)
            run('xps_tsne_descent_f64', [pr], max_iter - it, max_iter, momentum, exag, 300, 1e-7)
            assert all(b.guards_intact() for b in pr['_bufs'])
            head = state_half(pr, (max_iter - it) & 1)
            assert head['done'] == 1.0 and head['it'] == max_iter - 1
            Yin = pr['Y_out'].cpu().numpy().copy()
            t += max_iter - it
            gap = float(np.abs(Yin - runs[np.float64][t]).max())
            scale = float(np.abs(Yin).max())
            print(f'{name} nc={nc} plan={len(plan)} launch {t + 1}: gap {gap:.3e} = {gap / scale:.2e} of the scale, bar {bars[t]:.3e}, '
                  f'ratio {gap / bars[t]:.2e}')
            assert gap <= bars[t]


# ------------------------------------------------------------------------------------------------ refusals
def test_every_refusal_is_invalid_before_any_launch():
    la, lib = LA(), LIB()
    name = 'n5_D3'
    dv = device_affinities(name)
    n = 5

    def refused(entry, probs, *args, tab_edit=None, tiles_edit=None, ws_bytes=None, null_ws=False):
        tab, tiles = la.tsne_table(probs), la.tsne_tiles([p['n'] for p in probs])
        if tab_edit:
            tab_edit(tab)
        if tiles_edit is not None:
            tiles = tiles_edit(tiles)
        nb = int(getattr(lib.lib(), entry + '_workspace')(len(probs), max(len(tiles), 1)))
        ws = Buf64(max(nb // 8, 1))
        with pytest.raises(lib.XpsError, match=r'code -1'):
            lib.call(entry, tab.ctypes.data, len(probs), tiles.ctypes.data, len(tiles), *args, 0 if null_ws else ws.ptr,
                     nb if ws_bytes is None else ws_bytes, la.stream())
        torch.cuda.synchronize()
        assert ws.untouched()
        for p in probs:
            assert all(b.untouched() for b in p.get('_bufs', []))

    def word(w, v):
        def edit(tab):
            tab[w] = v
        return edit

    sq = lambda: sqdist_problem(name)
    for kw in (dict(tab_edit=word(la.TS_N, 1)), dict(tab_edit=word(la.TS_N, la.TSNE_MAX_SAMPLES + 1)), dict(tab_edit=word(la.TS_NC, 3)),
               dict(tab_edit=word(la.TS_G, 0)), dict(tab_edit=word(la.TS_D2, 0)), dict(tab_edit=word(la.TS_LDG, n - 1)),
               dict(tiles_edit=lambda t: t + np.int32([0, 1])), dict(tiles_edit=lambda t: t + np.int32([1, 0])),
               dict(tiles_edit=lambda t: t - np.int32([1, 0])), dict(tiles_edit=lambda t: np.concatenate([t, t])),
               dict(tiles_edit=lambda t: t[:0].copy()), dict(ws_bytes=8), dict(null_ws=True)):
        refused('xps_tsne_sqdist_f32', [sq()], **kw)

    def aff():
        ap = affinity_buffers(n)
        ap['D2'] = torch.from_numpy(dv['d2']).cuda()
        return ap
    for perp in (0.0, -1.0, float('nan'), float('inf'), 5.0, 7.5):
        refused('xps_tsne_affinities_f64', [aff()], perp)
    for w in (la.TS_D2, la.TS_C, la.TS_P, la.TS_BETA, la.TS_STEPS, la.TS_ROWSUM):
        refused('xps_tsne_affinities_f64', [aff()], 2.0, tab_edit=word(w, 0))
    same = aff()
    refused('xps_tsne_affinities_f64', [same], 2.0, tab_edit=word(la.TS_C, same['P'].data_ptr()))
    refused('xps_tsne_affinities_f64', [aff()], 2.0, ws_bytes=8)

    Y0 = TR.random_init(n, 2, 1)
    ds = lambda **kw: descent_problem(name, Y0, 2, kw.get('it_begin', 0), kw.get('lr', 50.0))
    good = (3, 10, 0.5, 12.0, 300, 1e-7)
    for args in ((-1, 10, 0.5, 12.0, 300, 1e-7), (3, 0, 0.5, 12.0, 300, 1e-7), (3, 10, -0.5, 12.0, 300, 1e-7),
                 (3, 10, float('inf'), 12.0, 300, 1e-7), (3, 10, 0.5, 0.0, 300, 1e-7), (3, 10, 0.5, float('nan'), 300, 1e-7),
                 (3, 10, 0.5, 12.0, -1, 1e-7), (3, 10, 0.5, 12.0, 300, float('nan'))):
        refused('xps_tsne_descent_f64', [ds()], *args)
    refused('xps_tsne_descent_f64', [ds(it_begin=10)], *good)
    refused('xps_tsne_descent_f64', [ds(it_begin=-1)], *good)
    refused('xps_tsne_descent_f64', [ds(lr=0.0)], *good)
    refused('xps_tsne_descent_f64', [ds(lr=float('inf'))], *good)
    for w in (la.TS_P, la.TS_YIN, la.TS_YOUT, la.TS_STATE):
        refused('xps_tsne_descent_f64', [ds()], *good, tab_edit=word(w, 0))
    refused('xps_tsne_descent_f64', [ds()], *good, tab_edit=word(la.TS_NC, 0))
    refused('xps_tsne_descent_f64', [ds()], *good, ws_bytes=8)
    assert lib.lib().xps_tsne_descent_f64_workspace(0, 1) == 0 and lib.lib().xps_tsne_state_bytes(0) == 0
