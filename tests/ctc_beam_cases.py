"""The inputs on which the whole CTC beam is compared with the restatement (tests/test_gpu_ctc_beam_trace.py on the device,
tests/test_ctc_beam_host.py for what these inputs can tell apart).  The smallest shapes that reach each branch of
csrc/xps_ctc_beam.hip; float32 logits, the reference log-probs are their float64 log-softmax.

Stream s of a case is the case's input drawn with seed + s.  Every seed recorded here passes ctc_beam_ref.trace_is_robust for
streams 0 .. 7 (B8 cases) or 0 .. 2, as float64 log-probs and as their float32 roundings (but see F32_FRAMES_HELD); the host
test asserts it.  A seed that fails is replaced by another one of the same shape, here.  The restatement's search of every
stream is computed once (trace) and shared by all tests."""
import functools

import numpy as np

from ctc_beam_ref import beam_trace

#   name: (T, S, K, blank, seed, kind, scale of the normal logits)      what it reaches
GRID = {
    'random':     (12, 7, 16, 2, 100, 'normal', 2.5),    # both merge orders (k < j, j < k)
    'dupcols':    (10, 6, 12, 0, 200, 'dupcols', 2.0),   # column 2 = column 1, column 5 = column 4: exact ties decided by key
    'uniform':    (6, 5, 20, 0, 300, 'uniform', 0.0),    # ties everywhere, the parent-ends-in-last rule
    'neginf':     (8, 6, 8, 0, 400, 'neginf', 2.0),      # -inf scores, valid -inf candidates before invalid ones
    'sparse':     (9, 3, 128, 1, 500, 'normal', 1.0),    # the beam is never full (n_new < K), the smallest-key rule
    'k1':         (7, 5, 1, 0, 600, 'normal', 1.5),      # K = 1
    'blank_only': (4, 1, 3, 0, 700, 'uniform', 0.0),     # S = 1
    'off_512':    (5, 8, 64, 0, 800, 'normal', 1.5),     # offline n * S = 512: one candidate per thread and pass
    'off_513':    (5, 9, 57, 0, 900, 'normal', 1.5),     # offline 513: four
    'str_2048':   (4, 16, 128, 15, 1000, 'normal', 1.5),  # streaming 2048: one candidate per thread, two passes
    'str_2080':   (6, 40, 52, 0, 1100, 'normal', 1.5),   # streaming 2080: four
    'full':       (3, 64, 128, 63, 1200, 'normal', 3.0),  # 8192 candidates; blank in the last column, so child bits end at 62
    'bit63':      (3, 64, 100, 0, 1300, 'normal', 3.0),  # token 63 is no blank here: cmask bit 63
}
BOUNDARY = {'off_512': 64, 'off_513': 57, 'str_2048': 128, 'str_2080': 52}   # the member count n that n * S is meant for
B8 = ('k1', 'blank_only', 'uniform', 'neginf')          # the four cheapest cases: the only ones run with 8 streams
# The float32 roundings of the log-probs are robust as well, with one exception that no seed can mend: a uniform row rounded to
# float32.  After frame 3 (1, 1) and (1, 2, 1) have the same probability through different sums, equal bits in double and
# one ulp apart in long double: a coincidental tie.  The offline test holds that form to the restatement in the frames before.
F32_FRAMES_HELD = {'uniform': 3}


def dims(name):
    T, S, K, blank = GRID[name][:4]
    return T, S, K, blank


def n_streams_checked(name):
    return 8 if name in B8 else 3


def frames_held(name, f32=False):
    """Leading frames in which the restatement's order is the only one a correct search can give."""
    return F32_FRAMES_HELD.get(name, GRID[name][0]) if f32 else GRID[name][0]


@functools.lru_cache(maxsize=None)
def logits(name, stream=0):
    """(T, S) float32 logits of one stream of a case, read-only."""
    T, S, K, blank, seed, kind, scale = GRID[name]
    rng = np.random.default_rng(seed + stream)
    if kind == 'uniform':
        z = np.full((T, S), 0.25 * stream, np.float32)
    else:
        z = (rng.standard_normal((T, S)) * scale).astype(np.float32)
    if kind == 'dupcols':
        z[:, 2] = z[:, 1]
        z[:, 5] = z[:, 4]
    if kind == 'neginf':                     # never a whole row
        for t in range(0, T, 2):
            z[t, rng.integers(1, S)] = -np.inf
        z[3, blank] = -np.inf
    z.setflags(write=False)
    return z


def log_softmax64(x):
    """The kernels' row-wise fp64 log-softmax, (x - m) - log(sum exp(x - m)), on the host."""
    x = np.asarray(x, dtype=np.float64)
    m = x.max(-1, keepdims=True)
    return (x - m) - np.log(np.exp(x - m).sum(-1, keepdims=True))


@functools.lru_cache(maxsize=None)
def log_probs(name, stream=0, f32=False):
    """The reference log-probs of a stream; f32: rounded to float32 and widened again (the offline kernel's float32 input)."""
    lp = log_softmax64(logits(name, stream))
    if f32:
        lp = lp.astype(np.float32).astype(np.float64)
    lp.setflags(write=False)
    return lp


@functools.lru_cache(maxsize=None)
def trace(name, stream=0, f32=False):
    """The restatement's whole search of a stream, computed once and shared; nobody changes it."""
    T, S, K, blank = dims(name)
    return beam_trace(log_probs(name, stream, f32), K, blank)
