"""Plain-torch restatement of the StyleGAN2 ``Generator`` and ``Discriminator`` (stylegan2/model.py:402-581, 654-712), assembled
from the blocks the repository already pins to the reference: ``oracle.torch_ref`` (modulated_conv2d, upfirdn2d, fused_leaky_relu,
equal_linear, conv_layer, d_r1_loss) and ``mbstd_ref.minibatch_stddev``.  Differentiable to any order, runs in the dtype of its
parameter dictionary (the tests use f64, and f32 for the noise floor); tests/test_stylegan2_ref.py pins it to the reference's
recorded outputs (tests/golden/stylegan2_gen.npz, stylegan2_disc.npz).

``P`` is ``params_of(module)``: the module's own ``state_dict()`` with every tensor dense and cast, the parameters as leaves.
``record=[]`` collects the pre-activation of every leaky-ReLU site; ``fragile(record, tol)`` counts the units an evaluation within
``tol`` of the site's largest value could put on the other side of zero."""
import math

import torch

import mbstd_ref
import oracle.torch_ref as O

TAPS = (1, 3, 3, 1)


def params_of(module, dtype=torch.float64):
    """state_dict -> {key: dense tensor of ``dtype`` on the CPU}; every ``named_parameters`` key is a leaf that requires grad."""
    P = {k: v.detach().cpu().contiguous().to(dtype).clone() for k, v in module.state_dict().items()}
    for n, _ in module.named_parameters():
        P[n].requires_grad_(True)
    return P


def param_list(module, P):
    return [P[n] for n, _ in module.named_parameters()]


def l2_err(a, b, floor=0.0):
    """||a - b||_2 / max(||b||_2, floor) in f64: the error of the WHOLE tensor, direction included."""
    a, b = a.detach().double().cpu(), b.detach().double().cpu()
    assert a.shape == b.shape, (a.shape, b.shape)
    num, den = float((a - b).norm()), max(float(b.norm()), float(floor))
    if den == 0.0:
        return 0.0 if num == 0.0 else float("inf")
    return num / den


def fragile(record, tol):
    """Units with |v| <= tol * max|v| of their site, over all recorded leaky-ReLU sites."""
    return sum(int((v.abs() <= tol * float(v.abs().max())).sum()) for v in record)


def _act(pre, record):
    if record is not None:
        record.append(pre.detach())
    return O.fused_leaky_relu(pre, None)


def _chan(b):
    return b.reshape(1, -1, 1, 1)


# ------------------------------------------------------------------------------------------------- generator side
def mapping(P, z, lr_mlp=0.01, record=None):
    """PixelNorm, then the EqualLinear(lr_mul, fused_lrelu) stack ``style.1 .. style.n``."""
    x = z * torch.rsqrt(z.pow(2).mean(1, keepdim=True) + 1e-8)
    i = 1
    while f"style.{i}.weight" in P:
        x = _act(O.equal_linear(x, P[f"style.{i}.weight"], None, lr_mlp) + P[f"style.{i}.bias"] * lr_mlp, record)
        i += 1
    return x


def styled_conv(P, pre, x, style, noise, *, upsample=False, record=None):
    """Modulated 3x3 conv (with its blur when upsampling) + noise.weight * noise + bias, leaky-ReLU * sqrt(2)."""
    y = O.modulated_conv2d(x, style, P[f"{pre}.conv.weight"], P[f"{pre}.conv.modulation.weight"], P[f"{pre}.conv.modulation.bias"],
                           upsample=upsample, blur_taps=TAPS)
    y = y + P[f"{pre}.noise.weight"] * noise
    return _act(y + _chan(P[f"{pre}.activate.bias"]), record)


def to_rgb(P, pre, x, style, skip=None):
    """Modulated 1x1 conv without demodulation + bias, plus the skip upsampled by two (FIR gain 4, pads (2, 1))."""
    y = O.modulated_conv2d(x, style, P[f"{pre}.conv.weight"], P[f"{pre}.conv.modulation.weight"], P[f"{pre}.conv.modulation.bias"],
                           demodulate=False)
    y = y + P[f"{pre}.bias"]
    if skip is not None:
        y = y + O.upfirdn2d(skip, (O.make_kernel(TAPS) * 4).to(skip), up=2, pad=(2, 1))
    return y


def generator(P, size, styles, noise, *, input_is_latent=False, inject_index=None, truncation=1, truncation_latent=None, record=None):
    """(image, latent [B, n_latent, D]).  ``styles``: one or two [B, D] (or one [B, n_latent, D]); ``noise``: one [B | 1, 1, H, W] per
    layer.  EVERY layer reads ``latent[:, i]``: the image is a function of the returned latent."""
    log_size = int(math.log2(size))
    n_latent = 2 * log_size - 2
    if not input_is_latent:
        styles = [mapping(P, s, record=record) for s in styles]
    if truncation < 1:
        styles = [truncation_latent + truncation * (s - truncation_latent) for s in styles]
    if len(styles) == 1:
        latent = styles[0] if styles[0].ndim == 3 else styles[0].unsqueeze(1).expand(-1, n_latent, -1)
    else:
        latent = torch.cat([styles[0].unsqueeze(1).expand(-1, inject_index, -1),
                            styles[1].unsqueeze(1).expand(-1, n_latent - inject_index, -1)], 1)
    b = latent.shape[0]
    out = P["input.input"].expand(b, -1, -1, -1)
    out = styled_conv(P, "conv1", out, latent[:, 0], noise[0], record=record)
    skip = to_rgb(P, "to_rgb1", out, latent[:, 1])
    for j in range(log_size - 2):
        out = styled_conv(P, f"convs.{2 * j}", out, latent[:, 2 * j + 1], noise[2 * j + 1], upsample=True, record=record)
        out = styled_conv(P, f"convs.{2 * j + 1}", out, latent[:, 2 * j + 2], noise[2 * j + 2], record=record)
        skip = to_rgb(P, f"to_rgbs.{j}", out, latent[:, 2 * j + 3], skip)
    return skip, latent


def path_regularize(image, latents, mean_path_length, img_noise, decay=0.01):
    """stylegan2/train.py:85-98 on [B, n_latent, D] latents (oracle.torch_ref.g_path_regularize is its [B, C] form): lengths =
    sqrt(mean over the latent axis of the squared norm over D).  Returns (penalty, mean, lengths)."""
    n = img_noise / math.sqrt(image.shape[2] * image.shape[3])
    (grad,) = torch.autograd.grad((image * n).sum(), latents, create_graph=True)
    lengths = torch.sqrt(grad.pow(2).sum(2).mean(1))
    mean = mean_path_length + decay * (lengths.mean() - mean_path_length)
    return (lengths - mean).pow(2).mean(), mean.detach(), lengths


# ------------------------------------------------------------------------------------------------- discriminator side
def conv_layer_sg2(P, pre, x, k, *, downsample=False, record=None):
    """[Blur] -> EqualConv2d -> bias + leaky-ReLU * sqrt(2): oracle.torch_ref.conv_layer up to the conv, then the recorded site."""
    y = O.conv_layer(P, pre, x, k, downsample=downsample, bias=False, activate=False, blur_taps=TAPS)
    return _act(y + _chan(P[f"{pre}.{2 if downsample else 1}.bias"]), record)


def res_block_sg2(P, pre, x, *, record=None):
    """conv1 in -> in, conv2 in -> out behind blur + stride 2, 1x1 blur + stride-2 skip without bias or activation."""
    y = conv_layer_sg2(P, f"{pre}.conv1", x, 3, record=record)
    y = conv_layer_sg2(P, f"{pre}.conv2", y, 3, downsample=True, record=record)
    s = O.conv_layer(P, f"{pre}.skip", x, 1, downsample=True, bias=False, activate=False, blur_taps=TAPS)
    return (y + s) / math.sqrt(2)


def discriminator(P, size, x, *, record=None):
    """Stem, ResBlocks down to 4x4, minibatch stddev (group 4, one feature), final_conv (513 in), NCHW flatten, final_linear."""
    y = conv_layer_sg2(P, "convs.0", x, 1, record=record)
    for j in range(1, int(math.log2(size)) - 1):
        y = res_block_sg2(P, f"convs.{j}", y, record=record)
    y = mbstd_ref.minibatch_stddev(y, 4, 1)
    y = conv_layer_sg2(P, "final_conv", y, 3, record=record)
    y = y.reshape(y.shape[0], -1)
    y = _act(O.equal_linear(y, P["final_linear.0.weight"], None) + P["final_linear.0.bias"], record)
    return O.equal_linear(y, P["final_linear.1.weight"], P["final_linear.1.bias"])


d_r1_loss = O.d_r1_loss
