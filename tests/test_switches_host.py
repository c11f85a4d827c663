"""The XPS_* switches: one table in the library (csrc/xps_switches.h, xps_set_switch / xps_get_switch / xps_list_switches),
one in Python (_switches.py), one list of all of them in README.md.  No GPU: the library loads without one."""
import ctypes as C
import json
import os
import re
import subprocess
import sys

import pytest

from cross_patient_speech_decoding_amd import _build, _lib, _switches

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, 'cross_patient_speech_decoding_amd')
LIBRARY_DEFAULTS = {
    'XPS_GEMM_PRECISION': 1, 'XPS_GEMM_SMALL_TILE_BLOCKS': 2048, 'XPS_GEMM_LONGK_128': 1, 'XPS_GEMM_BIG': 1, 'XPS_GEMM_DMA': 1,
    'XPS_PROJ_WS': 1, 'XPS_GEMM_BIG_DEEP': 0, 'XPS_GEMM_BIG_MIN_TILES': 192, 'XPS_GEMM_BIG_TAIL': 1, 'XPS_TN_BLOCKS': 512,
    'XPS_TN_UNIFORM': 0, 'XPS_GEMM_BIG_DEEP_TN': 0, 'XPS_TN_REDUCE': 0, 'XPS_GRU_STEP_PATH': 1, 'XPS_GRU_CLUSTER': 2,
    'XPS_GRU_CL_CUS': 0, 'XPS_GRU_CL2': 0, 'XPS_GRU_XIMG': 1, 'XPS_GRU_XOUT': 0}
PYTHON_DEFAULTS = {
    'XPS_FUSED_DROPOUT': 1, 'XPS_SPLIT4': 1, 'XPS_HPREV_SPLIT': 1, 'XPS_FWD_YSPLIT': 1, 'XPS_FWD_IMAGES': 0, 'XPS_SPLIT4_WEIGHTS': 1,
    'XPS_SPLIT4_WEIGHTS_MIN': 1 << 19, 'XPS_SKINNY_DX': 0, 'XPS_OVERLAP_WGRAD': 1, 'XPS_SIDE_PRIORITY': 'low', 'XPS_DECODER_WIDE': 1,
    'XPS_DP_OVERLAP': 1, 'XPS_TOPK_ORTHO': 'chol', 'XPS_MCCA_WHITEN': 'chol'}


@pytest.fixture(scope='module')
def lib():
    _build.build(verbose=False)
    return _lib.lib()


def fresh_process(**env):
    """Both tables as a new process sees them with `env` as its only XPS_* dispatch variables."""
    code = ('import json\n'
            'from cross_patient_speech_decoding_amd import _switches as s\n'
            'print("TABLES " + json.dumps([s.library_switches(), {n: s.get(n) for n in s._ROWS}]))\n')
    base = {k: v for k, v in os.environ.items() if not k.startswith('XPS_') or k == 'XPS_LIB_OVERRIDE'}
    r = subprocess.run([sys.executable, '-c', code], env=dict(base, **env), cwd=ROOT, capture_output=True, text=True, timeout=300)
    line = [ln for ln in r.stdout.splitlines() if ln.startswith('TABLES ')]
    assert line, r.stdout + r.stderr
    return json.loads(line[0][7:])


@pytest.fixture(scope='module')
def defaults(lib):
    return fresh_process()


def test_the_library_lists_exactly_its_19_rows_with_the_documented_defaults(defaults):
    assert defaults[0] == LIBRARY_DEFAULTS and list(defaults[0]) == list(LIBRARY_DEFAULTS)
    assert defaults[1] == PYTHON_DEFAULTS


def test_the_readme_table_names_every_switch_of_both_tables_with_its_default():
    with open(os.path.join(ROOT, 'README.md')) as f:
        rows = re.findall(r'^\| `(XPS_[A-Z0-9_]+)` \| ([^|]+) \| [^|]* \| (library|Python) \|', f.read(), flags=re.M)
    assert len(rows) == 33
    assert {n: d.strip() for n, d, w in rows if w == 'library'} == {n: str(d) for n, d in LIBRARY_DEFAULTS.items()}
    assert {n: d.strip() for n, d, w in rows if w == 'Python'} == {n: str(d) for n, d in PYTHON_DEFAULTS.items()}


def get(lib, name):
    v = C.c_longlong(-99)
    assert lib.xps_get_switch(name.encode(), C.byref(v)) == 0
    return v.value


@pytest.mark.parametrize('name,value', [('XPS_GEMM_DMA', 0), ('XPS_GEMM_BIG_DEEP', 1),          # booleans
                                        ('XPS_TN_BLOCKS', 768), ('XPS_GRU_CL_CUS', 64),        # integers
                                        ('XPS_GRU_CLUSTER', 1), ('XPS_TN_REDUCE', 2)])         # enumerated
def test_set_and_get_round_trip(lib, name, value):
    old = get(lib, name)
    try:
        assert lib.xps_set_switch(name.encode(), value) == 0
        assert get(lib, name) == value == _switches.get(name) == _switches.library_switches()[name]
    finally:
        assert lib.xps_set_switch(name.encode(), old) == 0
    assert get(lib, name) == old


def test_unknown_name_and_value_out_of_range_are_refused_with_a_message(lib):
    before = get(lib, 'XPS_GRU_CLUSTER')
    assert lib.xps_set_switch(b'XPS_GRU_CLUSTER', 3) == -1          # XPS_E_INVALID
    assert b'XPS_GRU_CLUSTER' in lib.xps_last_error() and b'3' in lib.xps_last_error()
    assert get(lib, 'XPS_GRU_CLUSTER') == before
    assert lib.xps_set_switch(b'XPS_NO_SUCH_SWITCH', 1) == -1
    assert b'XPS_NO_SUCH_SWITCH' in lib.xps_last_error()
    v = C.c_longlong()
    assert lib.xps_get_switch(b'XPS_NO_SUCH_SWITCH', C.byref(v)) == -1 and lib.xps_last_error()
    for name, bad in [('XPS_GEMM_DMA', 2), ('XPS_GEMM_DMA', -1), ('XPS_GEMM_BIG_MIN_TILES', 0), ('XPS_GEMM_PRECISION', 2)]:
        assert lib.xps_set_switch(name.encode(), bad) == -1 and name.encode() in lib.xps_last_error()
    small = C.create_string_buffer(16)
    assert lib.xps_list_switches(small, 16) == -1


@pytest.mark.parametrize('row,setter,getter,values', [
    ('XPS_GEMM_PRECISION', 'xps_set_gemm_precision', 'xps_get_gemm_precision', (0, 1)),
    ('XPS_GEMM_BIG', 'xps_set_gemm_big_tiles', 'xps_get_gemm_big_tiles', (0, 1)),
    ('XPS_GRU_CL2', 'xps_set_gru_bptt_grid', 'xps_get_gru_bptt_grid', (1, 0)),
    ('XPS_GRU_CLUSTER', 'xps_set_gru_cluster_mode', 'xps_get_gru_cluster_mode', (0, 1, 2))])
def test_the_older_setter_pairs_are_views_of_their_rows(lib, row, setter, getter, values):
    old = get(lib, row)
    try:
        for v in values:
            assert getattr(lib, setter)(v) == 0
            assert get(lib, row) == v == getattr(lib, getter)()
        for v in values:
            assert lib.xps_set_switch(row.encode(), v) == 0
            assert getattr(lib, getter)() == v
        assert getattr(lib, setter)(values[-1] + 5) == -1 and getattr(lib, getter)() == values[-1]
    finally:
        assert lib.xps_set_switch(row.encode(), old) == 0


def test_the_environment_of_a_fresh_process_is_parsed_by_the_rules_of_each_row(defaults):
    got, py = fresh_process(XPS_GEMM_PRECISION='fp32', XPS_GRU_CLUSTER='steps', XPS_GEMM_DMA='0', XPS_GEMM_BIG_DEEP='1',
                            XPS_GEMM_SMALL_TILE_BLOCKS='-5', XPS_GEMM_BIG_MIN_TILES='0', XPS_TN_REDUCE='f',
                            XPS_SKINNY_DX='1', XPS_SPLIT4='0', XPS_TOPK_ORTHO='jacobi')
    want = dict(LIBRARY_DEFAULTS, XPS_GEMM_PRECISION=0, XPS_GRU_CLUSTER=1, XPS_GEMM_DMA=0, XPS_GEMM_BIG_DEEP=1, XPS_TN_REDUCE=1)
    assert got == want and got['XPS_GEMM_SMALL_TILE_BLOCKS'] == 2048 and got['XPS_GEMM_BIG_MIN_TILES'] == 192
    assert py == dict(PYTHON_DEFAULTS, XPS_SKINNY_DX=1, XPS_SPLIT4=0, XPS_TOPK_ORTHO='jacobi')
    # default-on rows are off only for 0, default-off rows on only for 1; words the rows do not know leave the default
    got, py = fresh_process(XPS_TN_REDUCE='l', XPS_GEMM_DMA='off', XPS_GEMM_BIG_DEEP='yes', XPS_GEMM_PRECISION='bf16x3',
                            XPS_GRU_CLUSTER='0', XPS_GRU_XOUT='1', XPS_GRU_XIMG='0', XPS_FWD_IMAGES='2', XPS_MCCA_WHITEN='eig')
    assert got == dict(LIBRARY_DEFAULTS, XPS_TN_REDUCE=2, XPS_GRU_CLUSTER=0, XPS_GRU_XOUT=1, XPS_GRU_XIMG=0)
    assert py == dict(PYTHON_DEFAULTS, XPS_MCCA_WHITEN='eig')
    got, _ = fresh_process(XPS_TN_REDUCE='x', XPS_GRU_CLUSTER='whatever', XPS_GEMM_PRECISION='fp16', XPS_GRU_CL_CUS='128')
    assert got == dict(LIBRARY_DEFAULTS, XPS_GRU_CL_CUS=128)


def test_an_environment_change_after_the_first_use_is_not_followed(lib, monkeypatch):
    before = get(lib, 'XPS_GEMM_DMA'), get(lib, 'XPS_GRU_XOUT'), _switches.get('XPS_SPLIT4')
    monkeypatch.setenv('XPS_GEMM_DMA', '0' if before[0] else '1')
    monkeypatch.setenv('XPS_GRU_XOUT', '0' if before[1] else '1')
    monkeypatch.setenv('XPS_SPLIT4', '0' if before[2] else '1')
    assert (get(lib, 'XPS_GEMM_DMA'), get(lib, 'XPS_GRU_XOUT'), _switches.get('XPS_SPLIT4')) == before


def test_override_restores_also_when_the_body_raises_and_set_drops_the_memo(lib):
    from cross_patient_speech_decoding_amd.nn_models import functional
    old = {n: _switches.get(n) for n in ('XPS_GEMM_DMA', 'XPS_SKINNY_DX', 'XPS_MCCA_WHITEN', 'XPS_GRU_CLUSTER')}
    with pytest.raises(ZeroDivisionError):
        with _switches.override(XPS_GEMM_DMA=0, XPS_SKINNY_DX=1, XPS_MCCA_WHITEN='eig', XPS_GRU_CLUSTER='off'):
            assert [_switches.get(n) for n in old] == [0, 1, 'eig', 0]
            assert get(lib, 'XPS_GEMM_DMA') == 0 and lib.xps_get_gru_cluster_mode() == 0
            1 / 0
    assert {n: _switches.get(n) for n in old} == old
    for name in ('XPS_SPLIT4', 'XPS_GEMM_DMA'):                       # a Python row and a library row
        functional._memo(('sentinel',), lambda: 1)
        assert ('sentinel',) in functional._memo_values
        _switches.set(name, _switches.get(name))
        assert not functional._memo_values


def test_unknown_names_and_bad_values_raise_in_python(lib):
    with pytest.raises(KeyError):
        _switches.get('XPS_NO_SUCH_SWITCH')
    with pytest.raises(ValueError, match='XPS_NO_SUCH_SWITCH'):
        _switches.set('XPS_NO_SUCH_SWITCH', 1)
    before = _switches.get('XPS_GEMM_DMA')
    with pytest.raises(KeyError):
        with _switches.override(XPS_GEMM_DMA=1 - before, XPS_NO_SUCH_SWITCH=1):
            pass
    assert _switches.get('XPS_GEMM_DMA') == before                      # nothing was changed on the way
    for name, bad in [('XPS_SPLIT4', 2), ('XPS_MCCA_WHITEN', 'qr'), ('XPS_SPLIT4_WEIGHTS_MIN', -1), ('XPS_GRU_CLUSTER', 3)]:
        with pytest.raises(ValueError, match=name):
            _switches.set(name, bad)


def test_the_environment_is_read_in_one_place_per_language():
    hits = []
    for d, _, files in os.walk(os.path.join(PKG, 'csrc')):
        for f in files:
            with open(os.path.join(d, f)) as fh:
                hits += [f] * fh.read().count('getenv(')
    assert hits == ['xps_api.hip']
    both = set()
    for d, _, files in os.walk(PKG):
        for f in files:
            if f.endswith('.py'):
                with open(os.path.join(d, f)) as fh:
                    src = fh.read()
                if re.search(r'os\.environ[^\n]*XPS_|XPS_[^\n]*os\.environ', src):
                    both.add(os.path.relpath(os.path.join(d, f), PKG))
    assert both <= {'_switches.py', '_lib.py'} and '_lib.py' in both       # (XPS_LIB_OVERRIDE; _switches.py reads by row name)
