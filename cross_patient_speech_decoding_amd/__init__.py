"""MI355X-native hot path of coganlab/cross_patient_speech_decoding: latent alignment
(CCA / MCCA / joint PCA), the seq2seq GRU trainer and the figure analyses' scores (alignment.metrics,
manifold.TSNE), behind the reference's own Python and sklearn's surfaces.  All arithmetic on the path runs in libxps.so (hand-written HIP for gfx950,
C ABI in include/xps.h); importing the package does not need a GPU, calling it does."""
__version__ = '0.1.0'

_SURROGATES = ('TME', 'fit_many', 'tme_surrogates')        # surrogates/tme.py, imported when first asked for


def __getattr__(name):
    if name in _SURROGATES:
        from . import surrogates
        return getattr(surrogates, name)
    raise AttributeError(f'module {__name__!r} has no attribute {name!r}')


def __dir__():
    return sorted(list(globals()) + list(_SURROGATES))
