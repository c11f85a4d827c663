"""Float64 CPU restatement of the encoder layer (nn.TransformerEncoderLayer: post-norm, ReLU, batch_first, no masks) and of the
Transformer / CNNTransformer classifiers, written from torch primitives.  It is the project's own test code (in the manner of
tests/ctc_beam_ref.py): the GPU tests hand it the dropout decisions the kernels made (``masks=``) and compare.

Layouts are the HIP path's: activations time-major, rows (s, b).  Dropout masks are {0, 1} tensors in the layout of each site:
  conv (T', B, F) | attention probabilities (B, n_head, S, S) | dropout1 / dropout2 (S * B, D) | feed-forward (S * B, dim_fc)
and a kept value is divided by 1 - p."""
import torch


def attention(qkv, B, S, n_head, mask=None, p=0.0):
    """qkv (S * B, 3 D), row s * B + b = q | k | v  ->  context (S * B, D).  mask (B, n_head, S, S) or None."""
    D = qkv.shape[-1] // 3
    dh = D // n_head
    q, k, v = (t.reshape(S, B, n_head, dh).permute(1, 2, 0, 3) for t in qkv.reshape(S, B, 3 * D).split(D, dim=-1))
    scores = (q / dh ** 0.5) @ k.transpose(-1, -2)
    prob = torch.softmax(scores - scores.max(dim=-1, keepdim=True).values.detach(), dim=-1)
    if mask is not None:
        prob = prob * mask.to(prob.dtype) / (1.0 - p)
    return (prob @ v).permute(2, 0, 1, 3).reshape(S * B, D)


def layer_norm(v, weight, bias, eps=1e-5):
    mean = v.mean(dim=-1, keepdim=True)
    var = ((v - mean) ** 2).mean(dim=-1, keepdim=True)
    return (v - mean) / torch.sqrt(var + eps) * weight + bias


def add_layer_norm(x, r, weight, bias, eps=1e-5, mask=None, p=0.0):
    if mask is not None:
        r = r * mask.to(r.dtype).reshape(r.shape) / (1.0 - p)
    return layer_norm(x + r, weight, bias, eps)


def encoder_layer(x, w, pre, B, S, n_head, masks=None, p=0.0, eps=1e-5):
    """x (S * B, D); w: name -> tensor; pre: e.g. 'transformer_encoder.layers.0.'; masks: (attn, drop1, ff, drop2) or None."""
    ma, m1, mf, m2 = masks if masks is not None else (None, None, None, None)
    qkv = x @ w[pre + 'self_attn.in_proj_weight'].T + w[pre + 'self_attn.in_proj_bias']
    ctx = attention(qkv, B, S, n_head, ma, p)
    a = ctx @ w[pre + 'self_attn.out_proj.weight'].T + w[pre + 'self_attn.out_proj.bias']
    x = add_layer_norm(x, a, w[pre + 'norm1.weight'], w[pre + 'norm1.bias'], eps, m1, p)
    h = torch.relu(x @ w[pre + 'linear1.weight'].T + w[pre + 'linear1.bias'])
    if mf is not None:
        h = h * mf.to(h.dtype).reshape(h.shape) / (1.0 - p)
    f = h @ w[pre + 'linear2.weight'].T + w[pre + 'linear2.bias']
    return add_layer_norm(x, f, w[pre + 'norm2.weight'], w[pre + 'norm2.bias'], eps, m2, p)


def model_forward(w, x, kind, n_head, num_layers, stride=1, activation=True, training=True, masks=None, p=0.0):
    """Logits (B, classes) of Transformer (kind 'tr', x (B, T, D)) or CNNTransformer (kind 'cnn', x (B, T, C)) from the
    state-dict tensors ``w`` (float64; parameters may require grad).  masks: the sites' masks in the order the HIP model draws
    them -- conv (cnn only), then attn, drop1, ff, drop2 per layer -- or None.  BatchNorm uses batch statistics when training
    (running statistics are not updated here)."""
    it = iter(masks) if masks is not None else None
    if kind == 'cnn':
        y = torch.nn.functional.conv1d(x.permute(0, 2, 1), w['temporal_conv.conv.weight'], w['temporal_conv.conv.bias'],
                                       stride=stride)
        y = torch.nn.functional.batch_norm(y, w['temporal_conv.bn.running_mean'].clone(), w['temporal_conv.bn.running_var'].clone(),
                                           w['temporal_conv.bn.weight'], w['temporal_conv.bn.bias'], training=training,
                                           momentum=0.1, eps=1e-5)
        if activation:
            y = torch.relu(y)
        z = y.permute(2, 0, 1)                                             # (T', B, D)
        if it is not None:
            z = z * next(it).to(z.dtype) / (1.0 - p)
    else:
        z = x.permute(1, 0, 2)
    S, B, D = z.shape
    z = z + w['positional_encoding.pos_encoding'][0, :S, :].unsqueeze(1)
    h = z.reshape(S * B, D)
    for layer in range(num_layers):
        lm = tuple(next(it) for _ in range(4)) if it is not None else None
        h = encoder_layer(h, w, f'transformer_encoder.layers.{layer}.', B, S, n_head, lm, p)
    pooled = h.reshape(S, B, D).mean(dim=0)
    return pooled @ w['fc.weight'].T + w['fc.bias']
