from .ctc_decoder import beam_decode_batch, beam_decode_torch, decode, greedy_decode_batch  # noqa: F401
from .realtime_nn_model import DenseClassifier, RealtimeRNNModel, StackedRNN, StreamingDecoder  # noqa: F401
from .realtime_pipeline import RealtimePipeline, feature_map_from  # noqa: F401
