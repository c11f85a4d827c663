"""Prove that a change left every kernel alone: compile csrc/*.hip of a parent revision and of the working tree with the
product flags and compare the gfx950 code objects: .text and .rodata byte for byte, the symbol table apart from the
__hip_cuid_<hash> symbol (a hash of the whole translation unit, host code included).  Needs hipcc and the LLVM tools
beside it; no GPU.

  python tools/compare_device_code.py [--parent REV] [--jobs N] [--keep DIR]

prints one line per translation unit (sha256 of .text and .rodata) and exits 1 if one differs."""
import argparse
import hashlib
import os
import re
import shutil
import subprocess
import sys
import tempfile
from concurrent.futures import ThreadPoolExecutor

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from cross_patient_speech_decoding_amd import _build  # noqa: E402

TARGET = 'hipv4-amdgcn-amd-amdhsa--gfx950'
CSRC = 'cross_patient_speech_decoding_amd/csrc'


def llvm_tool(name):
    hipcc = os.path.realpath(_build.hipcc_path())
    for d in (os.path.join(os.path.dirname(hipcc), '..', 'lib', 'llvm', 'bin'), os.path.join(os.path.dirname(hipcc), '..', 'llvm', 'bin'),
              '/opt/rocm/lib/llvm/bin', '/opt/rocm/llvm/bin'):
        p = os.path.join(d, name)
        if os.path.exists(p):
            return p
    p = shutil.which(name)
    if p:
        return p
    raise RuntimeError(name + ' not found')


def code_object(src, work, reuse=False):
    """compile one source, return the path of its unbundled gfx950 code object"""
    base = os.path.join(work, os.path.basename(src)[:-4])
    if reuse and os.path.exists(base + '.co'):
        return base + '.co'
    subprocess.check_call([_build.hipcc_path()] + _build.FLAGS + ['-c', '-o', base + '.o', src])
    subprocess.check_call([llvm_tool('llvm-objcopy'), '-O', 'binary', '--only-section=.hip_fatbin', base + '.o', base + '.fatbin'])
    if os.path.getsize(base + '.fatbin') == 0:                  # a translation unit without device code (host entry points only)
        open(base + '.co', 'wb').close()
        return base + '.co'
    subprocess.check_call([llvm_tool('clang-offload-bundler'), '--unbundle', '--type=o', '--targets=' + TARGET,
                           '--input=' + base + '.fatbin', '--output=' + base + '.co'])
    return base + '.co'


def section(co, name):
    if os.path.getsize(co) == 0:
        return b''
    out = co + name.replace('.', '_')
    subprocess.check_call([llvm_tool('llvm-objcopy'), '-O', 'binary', '--only-section=' + name, co, out])
    with open(out, 'rb') as f:
        return f.read()


def symbols(co):
    if os.path.getsize(co) == 0:
        return []
    txt = subprocess.check_output([llvm_tool('llvm-readelf'), '--symbols', '--wide', co], text=True)
    return [re.sub(r'^\s*\d+:', '', ln) for ln in txt.splitlines() if '__hip_cuid_' not in ln]


def notes(co):
    if os.path.getsize(co) == 0:
        return ''
    txt = subprocess.check_output([llvm_tool('llvm-readelf'), '--notes', co], text=True)
    return re.sub(r'__hip_cuid_[0-9a-f]+', '__hip_cuid_', txt)


def describe(tree, work, jobs, reuse=False):
    os.makedirs(work, exist_ok=True)
    srcs = sorted(os.path.join(tree, CSRC, f) for f in os.listdir(os.path.join(tree, CSRC)) if f.endswith('.hip'))
    with ThreadPoolExecutor(max_workers=jobs) as ex:
        cos = list(ex.map(lambda s: code_object(s, work, reuse), srcs))
    return {os.path.basename(s): (section(c, '.text'), section(c, '.rodata'), symbols(c), notes(c)) for s, c in zip(srcs, cos)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--parent', default='HEAD')
    ap.add_argument('--jobs', type=int, default=min(8, os.cpu_count() or 1))
    ap.add_argument('--keep', default=None, help='directory for the objects (default: a temporary one)')
    a = ap.parse_args()
    work = a.keep or tempfile.mkdtemp(prefix='xps_cmp_')
    os.makedirs(work, exist_ok=True)
    ptree = os.path.join(work, 'parent_tree')
    if not os.path.exists(ptree):
        os.makedirs(ptree)
        tar = subprocess.Popen(['git', '-C', ROOT, 'archive', a.parent, CSRC, 'include'], stdout=subprocess.PIPE)
        subprocess.check_call(['tar', '-x', '-C', ptree], stdin=tar.stdout)
        if tar.wait():
            raise RuntimeError('git archive failed')
    old = describe(ptree, os.path.join(work, 'parent'), a.jobs, reuse=True)     # --keep: the parent's objects serve every later run
    new = describe(ROOT, os.path.join(work, 'new'), a.jobs)
    bad = sorted(set(old) ^ set(new))
    for name in sorted(set(old) & set(new)):
        diff = [what for what, x, y in zip(('.text', '.rodata', 'symbols', '.note'), old[name], new[name]) if x != y]
        print('%-22s .text %s  .rodata %s  %s' % (name, hashlib.sha256(new[name][0]).hexdigest()[:16],
              hashlib.sha256(new[name][1]).hexdigest()[:16], 'DIFFERS: ' + ', '.join(diff) if diff else 'same'))
        if diff:
            bad.append(name)
    if not a.keep:
        shutil.rmtree(work, ignore_errors=True)
    print('%d translation units, %d differ' % (len(new), len(bad)))
    return 1 if bad else 0


if __name__ == '__main__':
    sys.exit(main())
