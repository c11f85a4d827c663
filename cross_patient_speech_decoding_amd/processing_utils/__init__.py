"""Electrode subsampling (the reference's processing_utils/grid_subsampling.py and spatial_avg_subsampling.py): index
generation on the host, spatial averaging and channel selection on the MI355X (csrc/xps_subsample.hip)."""
from . import grid_subsampling, spatial_avg_subsampling  # noqa: F401
from .grid_subsampling import grid_subsample_sig_channels, grid_susbsample_idxs, select_channels_sweep  # noqa: F401
from .spatial_avg_subsampling import (spatial_avg_data, spatial_avg_idxs, spatial_avg_sig_channels,  # noqa: F401
                                      spatial_avg_sweep)
