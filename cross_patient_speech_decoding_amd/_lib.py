"""ctypes binding of libxps.so (include/xps.h).  The product path has NO fallback: if
the library is missing or a call fails, an exception is raised."""
import ctypes as C
import os
import re

_PKG = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get('XPS_LIB_OVERRIDE') or os.path.join(_PKG, 'libxps.so')   # override: A/B builds in tools/
HEADER_PATH = os.path.join(_PKG, '..', 'include', 'xps.h')

_lib = None


class RowMap(C.Structure):
    """xps_rowmap: row i lives at (i // rpg) * gs + (i % rpg) * ld."""
    _fields_ = [('gs', C.c_int64), ('ld', C.c_int64), ('rpg', C.c_int32), ('fmt', C.c_int32)]


_rowmaps = {}


def rowmap(ld, rpg=1 << 30, gs=0, fmt=0):
    """xps_rowmap descriptor.  Instances are cached and shared (the library only reads them; embedding one in an
    xps_tn_problem copies it): building a ctypes struct costs ~2 us and a training step needs ~40 of them.
    fmt = 1 (XPS_FMT_SPLIT4): the GEMM input operand holds pre-split bf16 hi / lo groups (include/xps.h)."""
    key = (ld, rpg, gs, fmt)
    r = _rowmaps.get(key)
    if r is None:
        r = RowMap(int(gs), int(ld), int(rpg), int(fmt))
        if len(_rowmaps) < 4096:
            _rowmaps[key] = r
    return r


class TnProblem(C.Structure):
    """xps_tn_problem"""
    _fields_ = [('A', C.c_void_p), ('B', C.c_void_p), ('C', C.c_void_p), ('colsum_a', C.c_void_p),
                ('ra', RowMap), ('rb', RowMap), ('rc', RowMap),
                ('M', C.c_int32), ('N', C.c_int32), ('K', C.c_int32), ('accumulate', C.c_int32)]


class XpsError(RuntimeError):
    pass


_CTYPES = {'int': C.c_int, 'int32_t': C.c_int32, 'int64_t': C.c_int64, 'uint64_t': C.c_uint64, 'size_t': C.c_size_t,
           'float': C.c_float, 'double': C.c_double, 'long long': C.c_longlong}
_POINTEES = set(_CTYPES) | {'void', 'char', 'unsigned', 'uint8_t', 'xps_rowmap', 'xps_tn_problem'}


_NAME = re.compile(r'\b(xps_[a-z0-9_]+)\s*\(')


def _strip(src):
    """Header text without its /* */ comments (the header has no // comments; a name in one would count as declared)."""
    return re.sub(r'/\*.*?\*/', '', src, flags=re.S)


def _ctype(decl, fn, is_return=False):
    """ctypes class of one C parameter or return type.  `const` and the parameter's name are noise; anything else the
    header has not used before (a new type, an array declarator) raises, naming the function: nothing is guessed."""
    words = re.sub(r'\bconst\b', ' ', decl).replace('*', ' * ').split()
    what = ' '.join(words)
    if not is_return and len(words) > 1 and words[-1] != '*':
        if not re.fullmatch(r'[A-Za-z_]\w*', words.pop()):          # the parameter's name
            raise XpsError(f'include/xps.h: {fn}: cannot read the parameter {what!r}')
    base, stars = ' '.join(w for w in words if w != '*'), words.count('*')
    if stars == 0 and base in _CTYPES:
        return _CTYPES[base]
    if stars == 1 and base == 'xps_rowmap':
        return C.POINTER(RowMap)
    if stars == 1 and base == 'char' and is_return:
        return C.c_char_p
    if stars and base in _POINTEES:                  # device pointers, host arrays of them, void**, xps_tn_problem*
        return C.c_void_p
    raise XpsError(f'include/xps.h: {fn}: no ctypes mapping for the C type in {what!r}')


def parse_signatures(src):
    """name -> (restype, [argtypes]) of every `ret xps_name(args);` in the header text `src`, /* */ comments and
    preprocessor lines stripped.  Raises for a declaration _ctype cannot read and for an xps_ name followed by `(` that no
    prototype was read for, so no entry point is bound wrongly or left unbound silently."""
    src = re.sub(r'^[ \t]*#.*$', '', _strip(src), flags=re.M)
    sigs = {}
    for ret, fn, args in re.findall(r'([A-Za-z_][\w\s\*]*?)\b(xps_[a-z0-9_]+)\s*\(([^()]*)\)\s*;', src):
        args = [] if args.strip() in ('', 'void') else args.split(',')
        sigs[fn] = (_ctype(ret, fn, is_return=True), [_ctype(a, fn) for a in args])
    unread = sorted(set(_NAME.findall(src)) - set(sigs))
    if unread:
        raise XpsError(f'include/xps.h: no prototype could be read for {unread}')
    return sigs


def header_functions(path=HEADER_PATH):
    """Names of all functions declared in include/xps.h."""
    with open(path) as f:
        return sorted(set(_NAME.findall(_strip(f.read()))))


def _header_signatures():
    if not os.path.exists(HEADER_PATH):
        raise XpsError(f'{HEADER_PATH} is missing: the ctypes signatures of libxps.so are read from it')
    with open(HEADER_PATH) as f:
        return parse_signatures(f.read())


SIGNATURES = _header_signatures()        # the header is the only place the argument types are written down


def lib():
    """Load libxps.so once.  Raises if it is not built — there is no CPU fallback."""
    global _lib
    if _lib is None:
        if not os.path.exists(LIB_PATH):
            raise XpsError(f'{LIB_PATH} is missing: run `python -c "import __graft_entry__ as g; g.build()"` '
                           '(hipcc --offload-arch=gfx950).  The HIP path has no CPU fallback.')
        # torch bundles its own HIP runtime (torch/lib/libamdhip64.so, same SONAME as the system
        # one).  It must be loaded FIRST so that libxps.so binds to the runtime that owns torch's
        # device context and streams; two runtimes in one process see "no ROCm-capable device".
        import torch  # noqa: F401
        l = C.CDLL(LIB_PATH)
        for name, (res, args) in SIGNATURES.items():
            fn = getattr(l, name)
            fn.restype, fn.argtypes = res, args
        _lib = l
    return _lib


def check(rc, what=''):
    if rc != 0:
        msg = lib().xps_last_error()
        raise XpsError(f'{what} failed (code {rc}): {msg.decode() if msg else "?"}')


_fns = {}


def call(name, *args):
    """Call an int-returning entry point and raise on a non-zero code.  (The bound functions are cached: a training step makes
    ~45 of these calls and the host path is as long as the GPU's.)"""
    fn = _fns.get(name)
    if fn is None:
        fn = _fns[name] = getattr(lib(), name)
    rc = fn(*args)
    if rc:
        check(rc, name)
