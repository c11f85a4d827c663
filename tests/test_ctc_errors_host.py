"""Edit-operation alignment without a device: the numpy restatement of xps_edit_align's contract (tests/ctc_errors_ref.py)
against a brute force over all monotone alignments, two hand-worked tie cases, and the host side of
realtime_sim/ctc_errors.py (its readouts on a hand-made result, every ValueError, the run-cutting arithmetic).  Every
quantity is an integer: every comparison is exact."""
import itertools

import numpy as np
import pytest
import torch

from ctc_errors_ref import DEL, HIT, INS, SUB, align_pair, edit_align_ref, monotone_alignments


def _ce():
    from cross_patient_speech_decoding_amd.realtime_sim import ctc_errors
    return ctc_errors


def _sequences(n_symbols, max_len):
    return [s for n in range(max_len + 1) for s in itertools.product(range(n_symbols), repeat=n)]


def test_restatement_equals_brute_force_over_all_monotone_alignments():
    """Every pair of sequences over 3 symbols with m, n <= 4 (121 sequences, 121^2 pairs): dist is the minimum cost over
    EVERY monotone alignment, the returned operations are a valid alignment of exactly that cost, and the count identities
    hold."""
    seqs = _sequences(3, 4)
    assert len(seqs) == 121
    by_len = {n: np.array([s for s in seqs if len(s) == n], np.int64).reshape(3 ** n, n) for n in range(5)}
    best = {}
    for m in range(5):
        for n in range(5):
            gaps, diag = monotone_alignments(m, n)
            A, T = by_len[m], by_len[n]
            neq = (A[:, None, :, None] != T[None, :, None, :]).reshape(len(A), len(T), m * n).astype(np.int64)
            cost = gaps[None, None, :] + neq @ diag.T                     # (pairs of A, pairs of T, every alignment)
            for x, a in enumerate(A):
                for y, t in enumerate(T):
                    best[tuple(a), tuple(t)] = int(cost[x, y].min())
    assert len(best) == 121 ** 2
    assert len(monotone_alignments(4, 4)[0]) == 321                      # the central Delannoy number D(4, 4)
    for (a, t), want in best.items():
        m, n = len(a), len(t)
        dist, counts, t2p, p2t, ops = align_pair(a, t)
        assert dist == want, (a, t)
        hits, subs, dels, ins = (int(c) for c in counts)
        assert hits + subs + dels == n and hits + subs + ins == m and subs + dels + ins == dist, (a, t)
        # the operations, read from the sequences' start, are a monotone alignment that uses every token once
        i = j = cost = 0
        for op, tj, pi in reversed(ops):
            if op in (HIT, SUB):
                assert (tj, pi) == (j, i) and (a[i] != t[j]) == (op == SUB), (a, t)
                assert t2p[j] == i and p2t[i] == j
                cost += op == SUB
                i, j = i + 1, j + 1
            elif op == INS:
                assert (tj, pi) == (-1, i) and p2t[i] == -1
                cost += 1
                i += 1
            else:
                assert op == DEL and (tj, pi) == (j, -1) and t2p[j] == -1
                cost += 1
                j += 1
        assert (i, j) == (m, n) and cost == want, (a, t)


def test_tie_case_ab_against_ba():
    """pred = ab, target = ba.  D[2][2] = 2 three ways (two substitutions; insert-hit-delete; delete-hit-insert): the
    diagonal is tested first at (2, 2) (D[1][1] + 1 = 2) and again at (1, 1), so both tokens are substituted."""
    dist, counts, t2p, p2t, ops = align_pair([0, 1], [1, 0])
    assert dist == 2 and counts.tolist() == [0, 2, 0, 0]
    assert t2p.tolist() == [0, 1] and p2t.tolist() == [0, 1]
    assert ops == [(SUB, 1, 1), (SUB, 0, 0)]


def test_tie_case_aa_against_a():
    """pred = aa, target = a.  D = [[0, 1], [1, 0], [2, 1]]: at (2, 1) the diagonal holds (D[1][0] + 0 = 1), so the SECOND a
    is the hit, and on the border j = 0 the first a is an insertion -- not the other way round."""
    dist, counts, t2p, p2t, ops = align_pair([0, 0], [0])
    assert dist == 1 and counts.tolist() == [1, 0, 0, 1]
    assert t2p.tolist() == [1] and p2t.tolist() == [-1, 0]
    assert ops == [(HIT, 0, 1), (INS, -1, 0)]
    # and the transposed pair: target aa, prediction a -- the second target token is hit, the first deleted
    dist, counts, t2p, p2t, _ = align_pair([0], [0, 0])
    assert dist == 1 and counts.tolist() == [1, 0, 1, 0] and t2p.tolist() == [-1, 0] and p2t.tolist() == [1]


# ---- the wrapper's readouts on a hand-made result ------------------------------------------------------------------------------
def _hand_made():
    """Three pairs over K = 4 classes, worked by hand:
       b = 0: pred 0 1 2    target 0 3 2    hit, substitution (3 -> 1), hit
       b = 1: pred 1        target 1 2      hit, deletion of 2
       b = 2: pred 3 0 0    target 0        insertion of 3, insertion of 0, hit (the LAST 0: the tie rule)"""
    ce = _ce()
    pred = torch.tensor([[0, 1, 2], [1, -1, -1], [3, 0, 0]])
    tgt = torch.tensor([[0, 3, 2], [1, 2, -1], [0, -1, -1]])
    pl, tl = torch.tensor([3, 1, 3]), torch.tensor([3, 2, 1])
    ref = edit_align_ref(pred.numpy(), pl.numpy(), tgt.numpy(), tl.numpy(), n_classes=4)
    assert ref[0].tolist() == [1, 1, 2] and ref[1].tolist() == [[2, 1, 0, 0], [1, 0, 1, 0], [1, 0, 0, 2]]
    assert ref[2].tolist() == [[0, 1, 2], [0, -1, -2], [2, -2, -2]] and ref[3].tolist() == [[0, 1, 2], [0, -2, -2], [-1, -1, 0]]
    conf = np.zeros((5, 5), np.int64)
    conf[0, 0], conf[3, 1], conf[2, 2], conf[1, 1], conf[2, 4], conf[4, 3], conf[4, 0] = 2, 1, 1, 1, 1, 1, 1
    assert np.array_equal(ref[4], conf)
    ea = ce.EditAlignment(*(torch.from_numpy(r) for r in ref), pred, pl, tgt, tl)
    return ea, conf


def test_readouts_on_a_hand_made_case():
    ea, conf = _hand_made()
    assert ea.hits.tolist() == [2, 1, 1] and ea.substitutions.tolist() == [1, 0, 0]
    assert ea.deletions.tolist() == [0, 1, 0] and ea.insertions.tolist() == [0, 0, 2]
    assert ea.target_ops().tolist() == [[0, 1, 0], [0, 2, -1], [0, -1, -1]]
    # positions 0, 1, 2 are reached by 3, 2, 1 targets, of which 0, 2, 0 were substituted or deleted
    assert ea.position_error_rate().tolist() == [0.0, 1.0, 0.0]
    # 4 errors over 6 target tokens; per_device's expression
    assert ea.per().dtype == torch.float64 and ea.per().dim() == 0
    assert float(ea.per()) == float(torch.tensor(4).double() / torch.tensor(6).double() * 100)
    assert ea.rates().tolist() == [1 / 6, 1 / 6, 2 / 6]
    assert ea.pairs(0) == [('hit', 0, 0), ('substitution', 3, 1), ('hit', 2, 2)]
    assert ea.pairs(1) == [('hit', 1, 1), ('deletion', 2, None)]
    assert ea.pairs(2) == [('insertion', None, 3), ('insertion', None, 0), ('hit', 0, 0)]


def test_rates_add_up_to_per_where_the_divisions_are_exact():
    """8 target tokens: every share is a multiple of 1/8, so the three rates add up to per() / 100 without rounding."""
    ce = _ce()
    pred = torch.tensor([[1, 1, 1, 1, 1], [0, 1, 2, 3, 9]])
    tgt = torch.tensor([[1, 2, 3, 0], [0, 1, 2, 3]])
    pl, tl = torch.tensor([2, 5]), torch.tensor([4, 4])
    ref = edit_align_ref(pred.numpy(), pl.numpy(), tgt.numpy(), tl.numpy())
    ea = ce.EditAlignment(*(torch.from_numpy(r) for r in ref[:4]), None, pred, pl, tgt, tl)
    assert ea.distance.tolist() == [3, 1]
    r = ea.rates()
    assert r.tolist() == [1 / 8, 2 / 8, 1 / 8]
    assert float(r[0] + r[1] + r[2]) == float(ea.per()) / 100 == 0.5


def test_confusion_by_folds_rows_and_columns_and_keeps_the_slots():
    ea, conf = _hand_made()
    folded = ea.confusion_by([0, 0, 1, 1])                               # classes {0, 1} -> 0, {2, 3} -> 1
    want = np.zeros((3, 3), np.int64)
    want[0, 0] = conf[:2, :2].sum()
    want[0, 1], want[1, 0], want[1, 1] = conf[:2, 2:4].sum(), conf[2:4, :2].sum(), conf[2:4, 2:4].sum()
    want[0, 2], want[1, 2] = conf[:2, 4].sum(), conf[2:4, 4].sum()
    want[2, 0], want[2, 1] = conf[4, :2].sum(), conf[4, 2:4].sum()
    assert folded.dtype == torch.int64 and np.array_equal(folded.numpy(), want)
    assert want.tolist() == [[3, 0, 0], [1, 1, 1], [1, 1, 0]]
    assert int(folded.sum()) == int(conf.sum()) and int(folded[2, 2]) == 0
    assert torch.equal(ea.confusion_by([0, 1, 2, 3]), ea.confusion)      # the identity map folds nothing
    # the articulator map of the docstring: 9 phonemes, 0-based, to 4 articulators, 0-based
    from cross_patient_speech_decoding_amd.alignment.alignment_utils import _PHON_TO_ARTIC
    cmap = [_PHON_TO_ARTIC[p + 1] - 1 for p in range(9)]
    assert cmap == [0, 0, 1, 1, 2, 2, 2, 3, 3]
    with pytest.raises(ValueError, match='class_map of 3 entries for 4 classes'):
        ea.confusion_by([0, 1, 2])
    with pytest.raises(ValueError, match='negative class'):
        ea.confusion_by([0, -1, 0, 0])
    with pytest.raises(ValueError, match='expected integers'):
        ea.confusion_by([0.0, 1.0, 0.0, 0.0])
    ce = _ce()
    bare = ce.EditAlignment(ea.distance, ea.counts, ea.target_to_pred, ea.pred_to_target, None, ea.pred, ea.pred_lengths,
                            ea.targets, ea.target_lengths)
    with pytest.raises(ValueError, match='confusion was not computed'):
        bare.confusion_by([0, 0, 1, 1])


# ---- every ValueError of edit_align, raised before any device call (host tensors reach none) ----------------------------------
def _ok():
    return dict(pred=torch.tensor([[1, 2, 0], [2, 2, 2]]), pred_lengths=[2, 3], targets=torch.tensor([[1, 0], [2, 1]]),
                target_lengths=[1, 2])


VALUE_ERRORS = [
    (dict(pred=torch.zeros(3, dtype=torch.int64)), r'pred of shape \(3,\): expected two axes, \(B, P\)'),
    (dict(targets=torch.zeros(2, 2, 2, dtype=torch.int64)), r'targets of shape \(2, 2, 2\): expected two axes, \(B, L\)'),
    (dict(pred=torch.zeros(2, 3)), 'pred of dtype torch.float32: expected integers'),
    (dict(targets=torch.zeros(2, 2, dtype=torch.bool)), 'targets of dtype torch.bool: expected integers'),
    (dict(targets=torch.zeros(3, 2, dtype=torch.int64)), '2 predictions for 3 targets'),
    (dict(pred=torch.zeros(2, 65537, dtype=torch.int64)), 'edit alignment of up to 65537 against 2 tokens: the kernel supports 65536 against 1024'),
    (dict(targets=torch.zeros(2, 1025, dtype=torch.int64)), 'edit alignment of up to 3 against 1025 tokens'),
    (dict(pred_lengths=None), 'pred_lengths is needed'),
    (dict(pred_lengths=[2]), '1 pred_lengths for 2 sequences'),
    (dict(target_lengths=[1, 2, 2]), '3 target_lengths for 2 sequences'),
    (dict(pred_lengths=[2, 4]), r'pred_lengths outside 0\.\.3'),
    (dict(pred_lengths=[-1, 3]), r'pred_lengths outside 0\.\.3'),
    (dict(target_lengths=[1, 3]), r'target_lengths outside 0\.\.2'),
    (dict(n_classes=0), 'n_classes 0: a confusion matrix needs at least one class'),
    (dict(n_classes=2), r'prediction 0 holds the label 2 at position 1: outside 0\.\.1'),
    (dict(n_classes=3, targets=torch.tensor([[1, 0], [2, -4]])), r'target 1 holds the label -4 at position 1: outside 0\.\.2'),
    (dict(max_workspace_bytes=5), 'one pair of up to 3 against 2 tokens needs 6 bytes of workspace: above max_workspace_bytes = 5'),
]


@pytest.mark.parametrize('i', range(len(VALUE_ERRORS)))
def test_value_errors(i):
    kw, text = VALUE_ERRORS[i]
    with pytest.raises(ValueError, match=text):
        _ce().edit_align(**{**_ok(), **kw})


def test_labels_past_the_lengths_are_not_checked_and_host_tensors_raise():
    """With every check passed a host tensor is refused (there is no CPU fallback): the ValueErrors above came first.  The
    labels 0 at pred[0, 2] and targets[0, 1] lie past their lengths; n_classes = 3 takes the rest."""
    kw = _ok()
    kw['pred'][0, 2], kw['targets'][0, 1] = -1, 99
    with pytest.raises(RuntimeError, match='edit_align needs device tensors'):
        _ce().edit_align(**kw, n_classes=3)


def test_run_cutting_arithmetic():
    runs = _ce().workspace_runs
    assert runs(0, 47, 5, 1 << 30) == []
    assert runs(2048, 47, 5, 1 << 30) == [(0, 2048)]
    per = 512 * 64
    assert runs(2048, 512, 64, 2048 * per) == [(0, 2048)]
    assert runs(2048, 512, 64, 2048 * per - 1) == [(0, 1024), (1024, 2048)]         # two even runs, not 2047 + 1
    assert runs(7, 3, 2, 6) == [(b, b + 1) for b in range(7)]                       # one pair per run
    assert runs(7, 3, 2, 17) == [(0, 2), (2, 4), (4, 6), (6, 7)]                    # 2 pairs fit: 4 runs
    assert runs(7, 3, 2, 18) == [(0, 3), (3, 6), (6, 7)]
    assert runs(10, 3, 2, 6 * 4) == [(0, 4), (4, 8), (8, 10)]                       # 3 runs of at most 4, evened: 4, 4, 2
    assert runs(5, 0, 9, 0) == [(0, 5)] and runs(5, 9, 0, 0) == [(0, 5)]            # no cells: no workspace, one run
    for B, P, L, cap in [(100, 47, 5, 1000), (33, 65536, 1024, 1 << 30), (9, 10, 10, 250)]:
        r = runs(B, P, L, cap)
        assert r[0][0] == 0 and r[-1][1] == B and all(a[1] == b[0] for a, b in zip(r, r[1:]))
        assert all((b1 - b0) * P * L <= cap for b0, b1 in r)
        assert len(r) == -(-B // (cap // (P * L)))                                  # as few runs as the limit allows
    with pytest.raises(ValueError, match='one pair of up to 65536 against 1024 tokens needs 67108864 bytes'):
        runs(1, 65536, 1024, (1 << 26) - 1)
