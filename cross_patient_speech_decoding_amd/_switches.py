"""The XPS_* dispatch switches (README.md, "Switches", is the one table of all of them).

The 14 rows below are the switches Python acts on: parsed from the environment once, at import.  The library keeps the
table of its own 19 (include/xps.h: xps_set_switch), filled from the environment when it is first used; get / set /
override forward a name that is not in _ROWS to it, and a name neither side knows raises.  A change inside a process
goes through set or override, never through os.environ."""
import contextlib
import ctypes as C
import os

from ._lib import XpsError, call, lib


def _on_unless_0(text):
    return 0 if text == '0' else 1


def _off_unless_1(text):
    return 1 if text == '1' else 0


def _word(default, other):
    return lambda text: other if text == other else default


_BOOL = (0, 1)
# name: (default, parse of the environment's text, values set() takes -- None: any integer >= 0)
_ROWS = {
    'XPS_FUSED_DROPOUT': (1, _on_unless_0, _BOOL),
    'XPS_SPLIT4': (1, _on_unless_0, _BOOL),
    'XPS_HPREV_SPLIT': (1, _on_unless_0, _BOOL),
    'XPS_FWD_YSPLIT': (1, _on_unless_0, _BOOL),
    'XPS_FWD_IMAGES': (0, _off_unless_1, _BOOL),
    'XPS_SPLIT4_WEIGHTS': (1, _on_unless_0, _BOOL),
    'XPS_SPLIT4_WEIGHTS_MIN': (1 << 19, int, None),
    'XPS_SKINNY_DX': (0, _off_unless_1, _BOOL),
    'XPS_OVERLAP_WGRAD': (1, _on_unless_0, _BOOL),
    'XPS_SIDE_PRIORITY': ('low', _word('low', 'default'), ('low', 'default')),
    'XPS_DECODER_WIDE': (1, _on_unless_0, _BOOL),
    'XPS_DP_OVERLAP': (1, _on_unless_0, _BOOL),
    'XPS_TOPK_ORTHO': ('chol', _word('chol', 'jacobi'), ('chol', 'jacobi')),
    'XPS_MCCA_WHITEN': ('chol', _word('chol', 'eig'), ('chol', 'eig')),
}
# words the library's enumerated rows may be set by (get returns the number)
_LIB_WORDS = {'XPS_GEMM_PRECISION': {'fp32': 0, 'bf16x3': 1}, 'XPS_GRU_CLUSTER': {'off': 0, 'steps': 1, 'persistent': 2},
              'XPS_TN_REDUCE': {'auto': 0, 'flat': 1, 'loop': 2}}

_values = {name: (parse(os.environ[name]) if name in os.environ else default) for name, (default, parse, _) in _ROWS.items()}
_hooks = []


def on_change(hook):
    """hook() runs after every set (functional drops its memoised predicates and workspace sizes there)."""
    _hooks.append(hook)


def get(name):
    v = _values.get(name)
    if v is not None:
        return v
    out = C.c_longlong()
    if lib().xps_get_switch(name.encode(), C.byref(out)) != 0:
        raise KeyError(f'{name}: neither a Python-side switch ({sorted(_ROWS)}) nor one of the library (xps_list_switches)')
    return out.value


def set(name, value):
    if name in _ROWS:
        allowed = _ROWS[name][2]
        value = int(value) if isinstance(value, bool) else value
        if (value not in allowed) if allowed else (not isinstance(value, int) or value < 0):
            raise ValueError(f'{name} takes {allowed or "an integer >= 0"}, not {value!r}')
        _values[name] = value
    else:
        try:
            call('xps_set_switch', name.encode(), int(_LIB_WORDS.get(name, {}).get(value, value)))
        except XpsError as e:
            raise ValueError(str(e)) from None
    for hook in _hooks:
        hook()


@contextlib.contextmanager
def override(**values):
    """with override(XPS_GEMM_DMA=0, XPS_SKINNY_DX=1): ...   -- the old values come back afterwards, also when the body raises."""
    old = {name: get(name) for name in values}          # (an unknown name raises here, before anything has changed)
    try:
        for name, value in values.items():
            set(name, value)
        yield
    finally:
        for name, value in old.items():
            set(name, value)


def library_switches():
    """name -> value of the library's rows, in the table's order."""
    buf = C.create_string_buffer(4096)
    call('xps_list_switches', buf, len(buf))
    return {k: int(v) for k, v in (line.split('=') for line in buf.value.decode().split())}
