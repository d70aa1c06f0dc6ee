"""Custom ops of the IDEAS hot path on hand-written gfx950 kernels (C ABI: include/ideas_hip.h).

Same public names as the reference's ``stylegan2.op`` (stylegan2/op/__init__.py:1-2) plus the conv family, the
discriminator's minibatch standard deviation, the generator's fused noise injection + bias + activation, the two image
transforms of adaptive discriminator augmentation, the two pieces of the LPIPS (VGG) distance the conv family does not cover, the
pools of the FID Inception-v3, the steganography codec (packed message bits <-> secret tensor, container image <-> 8-bit file), the
two small-step kernels of perceptual path length (path endpoints, pair preparation in front of the VGG), the channel attacks on
the 8-bit container (JPEG round trip, the JPEG file itself and its decoder; the PNG file; intensity, Gaussian noise, salt and pepper; Pillow-exact resize, Gaussian blur, median) and the
payload code (punctured convolutional
encoder, soft demapper, soft-decision Viterbi decoder).
"""
from .fused_act import FusedLeakyReLU, fused_leaky_relu
from .upfirdn2d import upfirdn2d
from .conv import conv2d, conv2d_bias_act, conv_transpose2d
from .modulated_conv import modulated_conv2d
from .minibatch_stddev import minibatch_stddev
from .noise_act import noise_bias_act
from .augment import affine_warp, color_affine
from .lpips import lpips_layer, max_pool2x2
from .pool import global_avg_pool, pool3x3
from .stego import bits_to_tensor, pack_bits, quantize_image, tensor_to_bits, unpack_bits
from .ppl import pair_prepare, path_endpoints
from .attack import jpeg_file_encode, jpeg_file_roundtrip, jpeg_files_to_host, jpeg_roundtrip, pixel_attack
from .png import png_file_encode, png_files_to_host
from .jpeg_decode import CorruptJpeg, JpegInfo, UnsupportedJpeg, jpeg_file_decode, jpeg_file_decode_grouped, parse_jpeg
from .resample import gaussian_blur_u8, median_u8, resample_tables, resize_u8
from .ecc import ecc_encode, ecc_soft, ecc_viterbi

__all__ = ["FusedLeakyReLU", "fused_leaky_relu", "upfirdn2d", "conv2d", "conv2d_bias_act", "conv_transpose2d", "modulated_conv2d",
           "minibatch_stddev", "noise_bias_act", "affine_warp", "color_affine", "max_pool2x2", "lpips_layer",
           "pool3x3", "global_avg_pool", "bits_to_tensor", "tensor_to_bits", "quantize_image", "pack_bits", "unpack_bits",
           "path_endpoints", "pair_prepare", "jpeg_roundtrip", "jpeg_file_roundtrip", "jpeg_file_encode", "jpeg_files_to_host", "pixel_attack", "png_file_encode", "png_files_to_host",
           "parse_jpeg", "JpegInfo", "UnsupportedJpeg", "CorruptJpeg", "jpeg_file_decode", "jpeg_file_decode_grouped", "resize_u8", "gaussian_blur_u8", "median_u8", "resample_tables",
           "ecc_encode", "ecc_soft", "ecc_viterbi"]
