from . import augmentations  # noqa: F401
from .ctc_align import CTCAlignment, forced_align, window_end_times  # noqa: F401
from .ctc_occupancy import CTCOccupancy, posterior_align  # noqa: F401
from .ctc_errors import EditAlignment, edit_align  # noqa: F401
from .ctc_decoder import beam_decode_batch, beam_decode_torch, decode, greedy_decode_batch, greedy_decode_device  # noqa: F401
from .realtime_datamodule import (CTCDataset, CTCHeldOutDataModule, CTCHeldOutTargetValAlignCVDataModule,  # noqa: F401
                                  CTCHeldOutTargetValAlignDataModule, CTCHeldOutTargetValCVDataModule,
                                  CTCHeldOutTargetValDataModule, align_to_target, reduce_to_latent_space, select_cv)
from .realtime_nn_model import (DenseClassifier, RealtimeRNNModel, StackedRNN, StreamingDecoder, calc_PER,  # noqa: F401
                                edit_distance, edit_distance_device, per_device)
from .realtime_pipeline import RealtimePipeline, feature_map_from  # noqa: F401
from .realtime_processing import process_HG_trials  # noqa: F401
from .session_replay import SessionReplay, SessionResult  # noqa: F401
