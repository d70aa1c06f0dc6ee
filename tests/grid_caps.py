"""The capped launches of ideas_amd/csrc/*.hip as a table.

A kernel whose grid is capped at a fixed number of workgroups covers the rest of its work in a grid-stride or tile loop, and only work
beyond ``cap x units`` sends a workgroup round that loop a second time: the stride expression, the 64-bit index arithmetic, a partial
last trip and the barrier at the top of a loop that keeps state in LDS matter from that trip on.  One row per capped launch site:

  file, site   the source file and the launcher or entry point whose launch the cap bounds
  line         the source line that holds the cap, as it stands in the file (leading blanks stripped)
  nth          which of the file's lines with that text (0: the first)
  cap          the number of workgroups in that line
  units        units of work one workgroup takes in one trip, and ``unit``: what a unit is
  test         ``file::test`` that runs the site with more than ``cap x units`` units of work

tests/test_grid_caps.py holds the rows against the sources (every cap is the literal, every capped launch of the forms the code base
uses is a row or an exclusion, every named test exists); the tests named here assert ``work > cap x units`` from their row where they
were written for it (tests/test_second_trip_gpu.py), and the comment of a row says how the figure follows where the test is an older one.
A new capped launch gets a row and a test that crosses it."""
from collections import namedtuple

Cap = namedtuple("Cap", "file site line nth cap units unit test")
ST = "tests/test_second_trip_gpu.py::"


def _row(file, site, line, cap, units, unit, test, nth=0):
    return Cap(file, site, line, nth, cap, units, unit, test)


GRID_16384 = "if (grid > 16384) grid = 16384;"
GRID_8192 = "if (grid > 8192) grid = 8192;"
GRID_4096 = "if (grid > 4096) grid = 4096;"
GRID_65536 = "if (grid > 65536) grid = 65536;"
TILE_GRID = "static unsigned tile_grid(int64_t ntiles) { return (unsigned)(ntiles < 65536 ? ntiles : 65536); }"

CAPS = {
    # ---- streaming and codec kernels: crossed by tests/test_second_trip_gpu.py, each test asserting its own excess from the row ----
    "pad.reflect_fold": _row("pad.hip", "ideas_reflect_fold", GRID_16384, 16384, 256, "channel vector of gx", ST + "test_reflect_fold"),
    "image_io.u8_to_f32": _row("image_io.hip", "ideas_image_u8_to_f32", GRID_8192, 8192, 256, "byte", ST + "test_image_u8_to_f32"),
    # stego.hip: one flat_grid() for four launches
    "stego.bits_to_tensor": _row("stego.hip", "ideas_bits_to_tensor", GRID_16384, 16384, 256, "element of z", ST + "test_bits_to_tensor"),
    "stego.image_flat_vec": _row("stego.hip", "image_to_u8_flat_kernel<T, true>", GRID_16384, 16384, 256 * 4, "quad of elements",
                                 ST + "test_image_f32_to_u8_flat_vector"),
    "stego.image_flat_elem": _row("stego.hip", "image_to_u8_flat_kernel<T, false>", GRID_16384, 16384, 256, "element",
                                  ST + "test_image_f32_to_u8_flat_element"),
    "stego.image_planar": _row("stego.hip", "image_to_u8_planar_kernel", GRID_16384, 16384, 256, "pixel", ST + "test_image_f32_to_u8_planar"),
    "attack.jpeg": _row("attack.hip", "launch_jpeg", GRID_16384, 16384, 4, "tile of 8 blocks", ST + "test_jpeg_roundtrip", nth=0),
    # launch_pixel: one cap line, the vector kernel takes quads of pixels and the element kernel pixels
    "attack.pixel_vec": _row("attack.hip", "launch_pixel", GRID_16384, 16384, 256 * 4, "pixel (four a thread)", ST + "test_pixel_attack_vector",
                             nth=1),
    "attack.pixel_elem": _row("attack.hip", "launch_pixel", GRID_16384, 16384, 256, "pixel", ST + "test_pixel_attack_element", nth=1),
    # attack_spatial.hip: one tile_grid() for both kernels, one tile a workgroup trip
    "attack_spatial.resample": _row("attack_spatial.hip", "launch_resample", TILE_GRID, 65536, 1, "tile", ST + "test_resample"),
    "attack_spatial.median": _row("attack_spatial.hip", "launch_median", TILE_GRID, 65536, 1, "tile", ST + "test_median"),
    # ecc.hip: one flat_grid() for the encoder and the demapper
    "ecc.encode": _row("ecc.hip", "ideas_ecc_encode", GRID_16384, 16384, 256, "coded byte", ST + "test_ecc_encode"),
    "ecc.soft": _row("ecc.hip", "ideas_ecc_soft", GRID_16384, 16384, 256, "message bit", ST + "test_ecc_soft"),
    # pool.hip: one pool3_grid() for the windows and the global average
    "pool.pool3x3": _row("pool.hip", "ideas_pool3x3_fwd", "if (g > 65536) g = 65536;", 65536, 256, "channel vector of a run of a row",
                         ST + "test_pool3x3"),
    "pool.global_avg": _row("pool.hip", "ideas_global_avg_pool", "if (g > 65536) g = 65536;", 65536, 256, "channel vector of a sample",
                            ST + "test_global_avg_pool"),
    "lpips.maxpool_fwd": _row("lpips.hip", "pool_grid", "if (nblk > 8192) nblk = 8192;", 8192, 256, "channel vector of an output pixel",
                              ST + "test_maxpool2x2_fwd"),
    "lpips.maxpool_bwd": _row("lpips.hip", "pool_grid", "if (nblk > 8192) nblk = 8192;", 8192, 256, "channel vector of a window",
                              ST + "test_maxpool2x2_bwd"),
    "upfirdn2d.generic": _row("upfirdn2d.hip", "upfirdn2d_impl", GRID_65536, 65536, 256, "output element", ST + "test_upfirdn2d_generic"),
    # ---- the remaining launches.  Where the named test is an older one, the comment works its figure out from the test's shapes ----
    # bias_act.hip, NHWC vector kernel: 256 threads x 4 float4 a trip in both variants
    "bias_act.vec": _row("bias_act.hip", "ideas_fused_bias_act", GRID_4096, 4096, 256 * 4, "float4 (not tiled: 1024 % C != 0)",
                         ST + "test_bias_act_vector_not_tiled", nth=0),
    # test_full_size_blur_and_bias_act_properties: fused_leaky_relu on f32 channels_last [32, 128, 256, 256]; C = 128 divides 1024, so
    # the tiled variant; n4 = 32 * 128 * 256 * 256 / 4 = 67 108 864 float4 > 4096 * 1024 = 4 194 304: 16 trips, forward and backward
    "bias_act.vec_tiled": _row("bias_act.hip", "ideas_fused_bias_act", GRID_4096, 4096, 256 * 4, "float4 (tiled: 1024 % C == 0)",
                               "tests/test_ops_gpu.py::test_full_size_blur_and_bias_act_properties", nth=1),
    "bias_act.scalar": _row("bias_act.hip", "ideas_fused_bias_act", GRID_8192, 8192, 256, "element", ST + "test_bias_act_scalar"),
    # one workgroup per 4096 elements by design (16 a thread: the loop runs at every size); past cap x units the cap binds
    "bias_act.channel_sum": _row("bias_act.hip", "ideas_channel_sum", "if (grid > 2048) grid = 2048;", 2048, 256 * 16, "element",
                                 ST + "test_channel_sum"),
    # conv_direct.hip, forward.  The pointwise kernels size their grids for 4 (rowdot) or 8 trips of a workgroup by design; units is the
    # whole of those trips at the test's channel counts, so past cap x units the cap binds and one more trip is made
    "conv_direct.rowdot": _row("conv_direct.hip", "conv_direct_impl", GRID_4096, 4096, 4 * 4 * 8, "pixel (64 / L = 8 a wave, 4 waves, 4 trips)",
                               ST + "test_conv_direct_forward"),
    "conv_direct.smallk_vec": _row("conv_direct.hip", "conv_direct_impl", GRID_8192, 8192, 64 * 8, "pixel (256 / (Cout / 4) = 64 a trip, 8 trips)",
                                   ST + "test_conv_direct_forward", nth=0),
    "conv_direct.smallk": _row("conv_direct.hip", "conv_direct_impl", GRID_8192, 8192, 42 * 8, "pixel (256 / Cout = 42 a trip, 8 trips)",
                               ST + "test_conv_direct_forward", nth=1),
    "conv_direct.direct": _row("conv_direct.hip", "conv_direct_impl", GRID_65536, 65536, 256, "output element", ST + "test_conv_direct_forward"),
    # conv_direct.hip, weight gradients: a workgroup takes a run of pixels (units, by design), longer once the cap binds
    "conv_direct.wgrad_vec": _row("conv_direct.hip", "wgrad_direct_impl", "if (blocks > 2048) blocks = 2048;", 2048, 2048, "pixel",
                                  ST + "test_conv_wgrad_direct", nth=0),
    "conv_direct.small_wgrad": _row("conv_direct.hip", "wgrad_direct_impl", "if (blocks > 1024) blocks = 1024;", 1024, 64, "pixel",
                                    ST + "test_conv_wgrad_direct"),
    "conv_direct.wgrad_direct": _row("conv_direct.hip", "wgrad_direct_impl", "if (blocks > 2048) blocks = 2048;", 2048, 256, "pixel",
                                     ST + "test_conv_wgrad_direct", nth=1),
    "conv_wino.fold": _row("conv_wino.hip", "ideas_wino_wgrad_fold",
                           "const int blocks = (int)(ideas_cdiv(n, 256) < 4096 ? ideas_cdiv(n, 256) : 4096);", 4096, 256, "element of dU",
                           ST + "test_wino_wgrad_fold"),
    # ---- rows an older test crosses by its own argument ----
    # MULTI_TRIP_CASES (1, 256, 47, 47) f32: 64 vectors a pixel, G = 64, 4 pixels a workgroup, 4 in flight: 16 a trip; 2209 pixels a
    # sample against 64 x 16: 3 trips (tests/test_lpips_gpu.py::_trips)
    "lpips.layer_fwd": _row("lpips.hip", "ideas_lpips_layer_fwd", "if (nblk > LP_MAX_BLOCKS) nblk = LP_MAX_BLOCKS;", 64, 16,
                            "pixel of a sample (at C = 256, f32)", "tests/test_lpips_gpu.py::test_lpips_layer_blocks_take_their_pixel_loop_more_than_once"),
    # MULTI_TRIP_CASES (5, 256, 82, 82) f32: 4 pixels a workgroup, 2 in flight: 8 a trip; 33 620 pixels against 4096 x 8 = 32 768
    "lpips.layer_bwd": _row("lpips.hip", "ideas_lpips_layer_bwd", "if (nblk > 4096) nblk = 4096;", 4096, 8, "pixel (at C = 256, f32)",
                            "tests/test_lpips_gpu.py::test_lpips_layer_blocks_take_their_pixel_loop_more_than_once"),
    # MULTI_TRIP (1, 132, 257, 257) f32: G = 64, 4 pixels a workgroup, 4 in flight: 16 a trip; 66 049 pixels against 4096 x 16 = 65 536
    # forward and 2048 x 16 backward (tests/test_stylegan2_gen_gpu.py::_trips)
    "noise_act.fwd": _row("noise_act.hip", "ideas_noise_bias_act", "const dim3 grid(na_grid(a, 4096));", 4096, 16, "pixel (at G = 64)",
                          "tests/test_stylegan2_gen_gpu.py::test_op_multi_trip_vs_f64"),
    "noise_act.bwd": _row("noise_act.hip", "ideas_noise_bias_act_bwd", "const dim3 grid(na_grid(a, NA_MAX_BLOCKS));", 2048, 16, "pixel (at G = 64)",
                          "tests/test_stylegan2_gen_gpu.py::test_op_multi_trip_vs_f64"),
    # CAPPED_CASE (4, 260, 9, 9, 1): 260 * 81 = 21 060 columns against 64 x 256 = 16 384 (tests/test_stylegan2_disc_gpu.py::_trips)
    "mbstd": _row("minibatch_stddev.hip", "mb_check", "if (nblk > MBSTD_MAX_BLOCKS) nblk = MBSTD_MAX_BLOCKS;", 64, 256, "column of a group",
                  "tests/test_stylegan2_disc_gpu.py::test_op_f32_capped_grid_walks_the_column_loop_twice"),
    # test_bwd_x asserts M * (K / 4) > 1024 * 256 for its two-split case itself
    "linear.fold": _row("linear.hip", "ideas_linear_bwd_x", "const unsigned fb = (unsigned)(n4 / 256 + 1 < 1024 ? n4 / 256 + 1 : 1024);", 1024, 256,
                        "float4 of gx", "tests/test_linear_abi_gpu.py::test_bwd_x"),
    # test_item_loops_that_run_twice asserts nblocks == 2048 and items > 2048 * 256 itself
    "weight_prep": _row("weight_prep.hip", "ideas_weight_prep_plan", "d->nblocks = (int)(items / 256 + 1 < 2048 ? items / 256 + 1 : 2048);", 2048,
                        256, "work item", "tests/test_weight_prep_gpu.py::test_item_loops_that_run_twice"),
    # n / 4 = 8192 * 256 + 2 lanes, the test says
    "optim.adam_ema": _row("optim.hip", "ideas_adam_ema", GRID_8192, 8192, 256, "float4 lane",
                           "tests/test_adam_ema_abi_gpu.py::test_adam_ema_second_trip_of_the_grid_stride_loop"),
    # 65 541 images of one luma and one chroma tile each against 16384 x 4
    "attack_jpeg": _row("attack_jpeg.hip", "grid_for", "return (unsigned)(grid > 16384 ? 16384 : grid);", 16384, 4, "tile",
                        "tests/test_jpeg_file_gpu.py::test_grid_stride_loop_turns_over"),
    # The persistent MFMA kernels: one tile a workgroup trip.  test_full_size_new_kernels_are_bitwise_the_kernels_they_replace runs
    # (c) the flat 1 x 1 split-bf16 kernel on 96 x 64 x 128 x 128 -> 128: M = 1 572 864 pixels in tiles of at most 128: >= 12 288 tiles
    # against 512; (e) the bf16 one on the same shape: tiles of at most 256 pixels, >= 6144 against 512; (d) the Winograd kernel on
    # 32 x 128 x 256 x 256 -> 128: 2 097 152 pixels, thousands of tiles against 256
    "conv_b3_pw": _row("conv_b3_pw.hip", "launch_pw", "const unsigned grid = (unsigned)(ntiles < 512 ? ntiles : 512);        // two persistent blocks per CU",
                       512, 1, "tile", "tests/test_ops_gpu.py::test_full_size_new_kernels_are_bitwise_the_kernels_they_replace"),
    "conv_bf16_pw": _row("conv_bf16_pw.hip", "launch_bf16_pw", "const unsigned grid = (unsigned)(ntiles < 512 ? ntiles : 512);", 512, 1, "tile",
                         "tests/test_ops_gpu.py::test_full_size_new_kernels_are_bitwise_the_kernels_they_replace"),
    "conv_b3_wino": _row("conv_b3_wino.hip", "go2", "const unsigned grid = (unsigned)(nt < 256 ? nt : 256);", 256, 1, "tile",
                         "tests/test_ops_gpu.py::test_full_size_new_kernels_are_bitwise_the_kernels_they_replace"),
}

# Hits of the completeness search (tests/test_grid_caps.py::FORMS) that are no caps of a launch.  Limits such as
# ``if (grid > 0x7fffffffLL) return IDEAS_E_SHAPE;`` and ``> MAXSEG`` are checks that assign nothing, and the search does not hit them.
#   (file, text the line contains): why
EXCLUDED = {
    ("attack_jpeg.hip", "(rem < 0 ? 1 : 0)"): "the rounding step of an integer division",
    ("stego.hip", "nbit - j0 < 8 ? nbit - j0 : 8"): "the message bits of one byte, in a kernel",
    ("linear.hip", "splits > 64 ? 64 : splits"): "the number of split-K slices: a second grid dimension, every slice one trip",
    ("noise_act.hip", "if (nblk > cap) nblk = cap;"): "na_grid's own parameter: its two call sites are the rows",
}
