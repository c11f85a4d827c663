from .models import (BaseLightningModel, CNNTransformer, CosineWarmupScheduler, DecoderRNN, EncoderRNN,  # noqa: F401
                     PositionalEncoding, Seq2SeqRNN, SimpleGRU, TCN_classifier, TemporalConv, TemporalConvRNN, Transformer,
                     cmat_acc)
