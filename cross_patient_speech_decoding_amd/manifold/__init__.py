"""Manifold learning on the MI355X behind sklearn's estimator surface: exact t-SNE, batched over data sets (tsne.py).
Importing needs no GPU; fitting does."""
from .tsne import TSNE  # noqa: F401
