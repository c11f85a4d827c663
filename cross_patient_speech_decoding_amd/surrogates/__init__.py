"""Surrogate data for the cross-patient controls: tensor maximum entropy surrogates on the device."""
from .tme import TME, fit_many, tme_surrogates

__all__ = ['TME', 'fit_many', 'tme_surrogates']
