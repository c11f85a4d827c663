"""Generate tests/golden/rsa.npz by running the REFERENCE's own representational dissimilarity analysis: the cell of
figure_analyses/fig_6.ipynb that defines calc_rdm_corr, compare_rdms, subset_rdm and cos_sim.

Run where a checkout of the reference is available:
    python tests/golden/make_rsa_fixtures.py <reference checkout>/aligned_decoding      (or REFERENCE_ALIGNED_DECODING=...)

The cell is read from the notebook at run time and executed in a namespace that holds what the notebook's import cell gives it
for these functions: numpy as np, scipy.stats as stats, the reference's alignment_utils as utils and its cnd_avg.  None of the
notebook's text is kept here or in the fixture; the fixture holds the seeded inputs (tests/rsa_ref.py's cases) and what the
reference's functions returned for them, with the library versions that computed it.
"""
import json
import os
import sys

import numpy as np
import scipy
from scipy import stats

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, '..'))
import rsa_ref as RR  # noqa: E402


def notebook_functions(ref):
    """The namespace left by the notebook's function-defining cell."""
    sys.path.insert(0, ref)
    import alignment.alignment_utils as utils                      # the reference's module
    with open(os.path.join(ref, 'figure_analyses', 'fig_6.ipynb')) as f:
        cells = json.load(f)['cells']
    source = [''.join(c['source']) for c in cells if c['cell_type'] == 'code' and 'def calc_rdm_corr' in ''.join(c['source'])]
    assert len(source) == 1, f'{len(source)} cells define calc_rdm_corr'
    ns = {'np': np, 'stats': stats, 'utils': utils, 'cnd_avg': utils.cnd_avg}
    exec(compile(source[0], 'fig_6.ipynb', 'exec'), ns)
    return ns


def main():
    ref = sys.argv[1] if len(sys.argv) > 1 else os.environ.get('REFERENCE_ALIGNED_DECODING')
    if not ref:
        sys.exit('usage: make_rsa_fixtures.py <reference checkout>/aligned_decoding')
    ns = notebook_functions(ref)
    out = {'versions': np.array([np.__version__, scipy.__version__])}
    names = sorted(RR.cases())
    out['names'] = np.array(names)
    rdms = {}
    for name in names:
        data, labels = RR.cases()[name]
        rdm, uniq = ns['calc_rdm_corr'](data, labels)
        rdms[name] = (rdm, uniq)
        out[f'{name}/data'], out[f'{name}/labels'] = data, labels
        out[f'{name}/rdm'], out[f'{name}/unique_labels'] = rdm, uniq
    pairs, pearson, cosine = [], [], []
    for i, a in enumerate(names):
        for b in names[i + 1:]:
            (ra, ua), (rb, ub) = rdms[a], rdms[b]
            shared = np.intersect1d(ua, ub)
            if len(shared) < 3:
                continue
            pairs.append((a, b))
            pearson.append(ns['compare_rdms'](ra, ua, rb, ub))
            ta = ns['subset_rdm'](ra, ua, shared)[np.triu_indices(len(shared), k=1)]
            tb = ns['subset_rdm'](rb, ub, shared)[np.triu_indices(len(shared), k=1)]
            cosine.append(ns['cos_sim'](ta, tb))
    out['pairs'], out['pearson'], out['cosine'] = np.array(pairs), np.array(pearson), np.array(cosine)
    # subset_rdm's rule: a shared label the RDM does not hold is dropped
    ra, ua = rdms[names[0]]
    asked = np.concatenate([ua[:3], ['no such label']])
    out['subset/asked'], out['subset/result'] = asked, ns['subset_rdm'](ra, ua, asked)
    path = os.path.join(HERE, 'rsa.npz')
    np.savez_compressed(path, **out)
    print(f'wrote {path}: {os.path.getsize(path)} bytes, {len(names)} data sets, {len(pairs)} comparisons')


if __name__ == '__main__':
    main()
