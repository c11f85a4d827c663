from .models import (BaseLightningModel, DecoderRNN, EncoderRNN, Seq2SeqRNN,  # noqa: F401
                     SimpleGRU, TCN_classifier, TemporalConv, TemporalConvRNN, cmat_acc)
