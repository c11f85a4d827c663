"""Latent alignment (CCA / MCCA / joint PCA / PCA) on the MI355X behind the reference's
sklearn-style surfaces.  Importing needs no GPU; fitting does."""
from .AlignCCA import AlignCCA, CCA_align  # noqa: F401
from .AlignMCCA import AlignMCCA  # noqa: F401
from .JointPCA import JointPCA  # noqa: F401
from .alignment_utils import cnd_avg, extract_group_conditions, label2str  # noqa: F401
from .pca import PCA, GramPCA, PCA_SPECTRUM_LIMIT, fit_many  # noqa: F401
from .fold_align import FoldAlignment, fit_folds, fit_folds_multi, fold_plan  # noqa: F401
from . import metrics  # noqa: F401
from .metrics import ClusterScores, cluster_scores, pt_corr, pt_corr_multi  # noqa: F401
from . import rsa  # noqa: F401
from .rsa import (RDMAlignment, RDMComparison, calc_rdm_corr, calc_rdm_corr_many, compare_rdms, compare_rdms_many,  # noqa: F401
                  cos_sim, rdm_alignment_scores, subset_rdm)
