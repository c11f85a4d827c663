from .cross_pt_decoders import (crossPtDecoder, crossPtDecoder_jointDimRed, crossPtDecoder_mcca,  # noqa: F401
                                crossPtDecoder_sepAlign, crossPtDecoder_sepDimRed)
from .svm import SVC  # noqa: F401,E402
from .bagging import BaggingClassifier  # noqa: F401,E402
from .search import SVCSearchCV  # noqa: F401,E402
from .fold_decode import FoldDecode, cross_val_decode  # noqa: F401,E402
from .aligned_search import AlignedSVCSearchCV  # noqa: F401,E402
