"""Seeded weights for the Transformer / CNNTransformer fixtures and tests: `weights_from_seed` with two corrections for these
models.  The positional table is a constant of the model, not a weight: ``positional_encoding.pos_encoding`` stays as
constructed.  LayerNorm gains are drawn around one: 1.0 is added to every ``norm1.weight`` / ``norm2.weight`` (the plain draw
would put them in +-0.1).  Data generation, not reference code."""
from weights import weights_from_seed


def transformer_weights_from_seed(state_dict, seed):
    out = weights_from_seed(state_dict, seed)
    for k, v in state_dict.items():
        if k.endswith('pos_encoding'):
            out[k] = v.clone()
        elif k.endswith('norm1.weight') or k.endswith('norm2.weight'):
            out[k] = out[k] + 1.0
    return out
