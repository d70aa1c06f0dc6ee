"""Launch-sequence pin of the modulated conv (op/modulated_conv.py), forward and backward, for every branch and flag set of its
autograd Function: same-resolution, upsampling, downsampling (chain, 1x1, fused launch), with and without demodulation, with the
bias + leaky-ReLU fused, following unfused, or absent.

Every op module reports a launch as ``_lib.check(rc, "name")``; the test replaces ``_lib.check`` by a recorder and compares the
names of one forward and one backward with a list written out below (``"--"`` stands between the two passes).  The lists are what
the shipped configuration produces (split-bf16 contraction, no IDEAS_* switch in the environment: the module is skipped otherwise).
Each case runs with four sets of trainable inputs -- everything, frozen weight, weight only, and everything inside ``grad_sink``
with pre-allocated ``.grad`` -- and asserts (a) the trace, (b) the gradients against the all-trainable run on the same inputs at
GTOL = 1e-4 (the bound of tests/test_modconv_down_gpu.py::test_frozen_weight_and_frozen_input), (c) what the node retains."""
import os

import pytest
import torch

from conftest import rel_err
from ideas_amd import _lib
from ideas_amd.op import conv as convmod
from test_bf16_gpu import bf16_mode  # noqa: F401  (the fixture)

pytestmark = pytest.mark.gpu
CL = torch.channels_last
GTOL = 1e-4
MODES = ("all", "frozen_w", "w_only", "sink")

if convmod.MATH != _lib.F32_B3 or any(k.startswith("IDEAS_") for k in os.environ):
    pytest.skip("the traces belong to the shipped configuration: split-bf16 math, no IDEAS_* switch set", allow_module_level=True)


# name: (mode, k, (B, Cin, Cout, H), demodulate, bias given, BLUR_CONV_MOD_MIN_BLOCKS or None)
CASES = {
    "same_act": ("same", 3, (2, 16, 32, 8), True, True, None),               # bias + activation in the conv epilogue
    "same": ("same", 3, (2, 16, 32, 8), True, False, None),
    "same_nodemod": ("same", 3, (2, 16, 32, 8), False, False, None),
    "torgb": ("same", 1, (2, 16, 3, 8), False, False, None),
    "same_cout30_bias": ("same", 3, (2, 16, 30, 8), True, True, None),       # cout % 4 != 0: the activation follows unfused
    "up": ("up", 3, (2, 16, 32, 8), True, False, None),
    "up_bias": ("up", 3, (2, 16, 32, 8), True, True, None),                  # blur_bias_act
    "up_nodemod": ("up", 3, (2, 16, 32, 8), False, False, None),
    "down_chain_act": ("down", 3, (2, 24, 32, 17), True, True, None),
    "down_chain": ("down", 3, (2, 24, 32, 17), True, False, None),
    "down_chain_nodemod": ("down", 3, (2, 24, 32, 17), False, False, None),
    "down_1x1": ("down", 1, (2, 16, 24, 12), True, False, None),
    "down_fused_act": ("down", 3, (4, 64, 128, 64), True, True, 0),          # the fused launch
}
BF16_CASES = ("same", "up")

# case -> trainable set -> entry points without their "ideas_" prefix, forward -- backward
EXPECTED = {"same_act": {"all": ["weight_sqsum", "demod", "weight_prep_plan", "weight_prep", "conv3x3_wino", "--", "act_bwd_dot", "weight_prep_plan",
                      "weight_prep", "conv3x3_wino", "pixel_dot", "weight_sqsum_f64", "demod_bwd", "conv3x3_wino_wgrad", "wino_wgrad_fold",
                      "demod_wgrad"],
              "frozen_w": ["weight_sqsum", "demod", "weight_prep_plan", "weight_prep", "conv3x3_wino", "--", "act_bwd_dot",
                           "weight_prep_plan", "weight_prep", "conv3x3_wino", "pixel_dot", "weight_sqsum_f64", "demod_bwd"],
              "w_only": ["weight_sqsum", "demod", "weight_prep_plan", "weight_prep", "conv3x3_wino", "--", "act_bwd_dot",
                         "weight_sqsum_f64", "demod_bwd", "conv3x3_wino_wgrad", "wino_wgrad_fold", "demod_wgrad"],
              "sink": ["weight_sqsum", "demod", "weight_prep_plan", "weight_prep", "conv3x3_wino", "--", "act_bwd_dot", "weight_prep_plan",
                       "weight_prep", "conv3x3_wino", "pixel_dot", "weight_sqsum_f64", "demod_bwd", "conv3x3_wino_wgrad", "wino_wgrad_fold",
                       "demod_wgrad"]},
 "same": {"all": ["weight_sqsum", "demod", "weight_prep_plan", "weight_prep", "conv3x3_wino", "--", "weight_prep_plan", "weight_prep",
                  "conv3x3_wino", "pixel_dot", "pixel_dot", "weight_sqsum_f64", "demod_bwd", "conv3x3_wino_wgrad", "wino_wgrad_fold",
                  "demod_wgrad"],
          "frozen_w": ["weight_sqsum", "demod", "weight_prep_plan", "weight_prep", "conv3x3_wino", "--", "weight_prep_plan", "weight_prep",
                       "conv3x3_wino", "pixel_dot", "pixel_dot", "weight_sqsum_f64", "demod_bwd"],
          "w_only": ["weight_sqsum", "demod", "weight_prep_plan", "weight_prep", "conv3x3_wino", "--", "pixel_dot", "weight_sqsum_f64",
                     "demod_bwd", "conv3x3_wino_wgrad", "wino_wgrad_fold", "demod_wgrad"],
          "sink": ["weight_sqsum", "demod", "weight_prep_plan", "weight_prep", "conv3x3_wino", "--", "weight_prep_plan", "weight_prep",
                   "conv3x3_wino", "pixel_dot", "pixel_dot", "weight_sqsum_f64", "demod_bwd", "conv3x3_wino_wgrad", "wino_wgrad_fold",
                   "demod_wgrad"]},
 "same_nodemod": {"all": ["weight_prep_plan", "weight_prep", "conv3x3_wino", "--", "weight_prep_plan", "weight_prep", "conv3x3_wino",
                          "pixel_dot", "demod_bwd", "conv3x3_wino_wgrad", "wino_wgrad_fold"],
                  "frozen_w": ["weight_prep_plan", "weight_prep", "conv3x3_wino", "--", "weight_prep_plan", "weight_prep", "conv3x3_wino",
                               "pixel_dot", "demod_bwd"],
                  "w_only": ["weight_prep_plan", "weight_prep", "conv3x3_wino", "--", "conv3x3_wino_wgrad", "wino_wgrad_fold"],
                  "sink": ["weight_prep_plan", "weight_prep", "conv3x3_wino", "--", "weight_prep_plan", "weight_prep", "conv3x3_wino",
                           "pixel_dot", "demod_bwd", "conv3x3_wino_wgrad", "wino_wgrad_fold"]},
 "torgb": {"all": ["weight_prep_plan", "weight_prep", "conv_igemm[b3]", "--", "conv_direct", "pixel_dot", "demod_bwd", "conv_wgrad_direct"],
           "frozen_w": ["weight_prep_plan", "weight_prep", "conv_igemm[b3]", "--", "conv_direct", "pixel_dot", "demod_bwd"],
           "w_only": ["weight_prep_plan", "weight_prep", "conv_igemm[b3]", "--", "conv_wgrad_direct"],
           "sink": ["weight_prep_plan", "weight_prep", "conv_igemm[b3]", "--", "conv_direct", "pixel_dot", "demod_bwd",
                    "conv_wgrad_direct"]},
 "same_cout30_bias": {"all": ["weight_sqsum", "demod", "weight_prep_plan", "weight_prep", "conv_igemm[b3]", "fused_bias_act", "--",
                              "fused_bias_act", "conv_direct", "pixel_dot", "pixel_dot", "weight_sqsum_f64", "demod_bwd",
                              "conv_wgrad_direct", "demod_wgrad"],
                      "frozen_w": ["weight_sqsum", "demod", "weight_prep_plan", "weight_prep", "conv_igemm[b3]", "fused_bias_act", "--",
                                   "fused_bias_act", "conv_direct", "pixel_dot", "pixel_dot", "weight_sqsum_f64", "demod_bwd"],
                      "w_only": ["weight_sqsum", "demod", "weight_prep_plan", "weight_prep", "conv_igemm[b3]", "fused_bias_act", "--",
                                 "fused_bias_act", "pixel_dot", "weight_sqsum_f64", "demod_bwd", "conv_wgrad_direct", "demod_wgrad"],
                      "sink": ["weight_sqsum", "demod", "weight_prep_plan", "weight_prep", "conv_igemm[b3]", "fused_bias_act", "--",
                               "fused_bias_act", "conv_direct", "pixel_dot", "pixel_dot", "weight_sqsum_f64", "demod_bwd",
                               "conv_wgrad_direct", "demod_wgrad"]},
 "up": {"all": ["weight_sqsum", "demod", "weight_prep_plan", "weight_prep", "weight_prep_plan", "weight_prep", "weight_prep_plan",
                "weight_prep", "weight_prep_plan", "weight_prep", "conv_igemm_multi", "upfirdn2d", "--", "upfirdn2d", "weight_prep_plan",
                "weight_prep", "conv_igemm[b3]", "pixel_dot", "pixel_dot", "weight_sqsum_f64", "demod_bwd", "conv_wgrad", "demod_wgrad"],
        "frozen_w": ["weight_sqsum", "demod", "weight_prep_plan", "weight_prep", "weight_prep_plan", "weight_prep", "weight_prep_plan",
                     "weight_prep", "weight_prep_plan", "weight_prep", "conv_igemm_multi", "upfirdn2d", "--", "upfirdn2d",
                     "weight_prep_plan", "weight_prep", "conv_igemm[b3]", "pixel_dot", "pixel_dot", "weight_sqsum_f64", "demod_bwd"],
        "w_only": ["weight_sqsum", "demod", "weight_prep_plan", "weight_prep", "weight_prep_plan", "weight_prep", "weight_prep_plan",
                   "weight_prep", "weight_prep_plan", "weight_prep", "conv_igemm_multi", "upfirdn2d", "--", "upfirdn2d", "pixel_dot",
                   "weight_sqsum_f64", "demod_bwd", "conv_wgrad", "demod_wgrad"],
        "sink": ["weight_sqsum", "demod", "weight_prep_plan", "weight_prep", "weight_prep_plan", "weight_prep", "weight_prep_plan",
                 "weight_prep", "weight_prep_plan", "weight_prep", "conv_igemm_multi", "upfirdn2d", "--", "upfirdn2d", "weight_prep_plan",
                 "weight_prep", "conv_igemm[b3]", "pixel_dot", "pixel_dot", "weight_sqsum_f64", "demod_bwd", "conv_wgrad", "demod_wgrad"]},
 "up_bias": {"all": ["weight_sqsum", "demod", "weight_prep_plan", "weight_prep", "weight_prep_plan", "weight_prep", "weight_prep_plan",
                     "weight_prep", "weight_prep_plan", "weight_prep", "conv_igemm_multi", "blur_fused", "--", "fused_bias_act",
                     "upfirdn2d", "weight_prep_plan", "weight_prep", "conv_igemm[b3]", "pixel_dot", "pixel_dot", "weight_sqsum_f64",
                     "demod_bwd", "conv_wgrad", "demod_wgrad"],
             "frozen_w": ["weight_sqsum", "demod", "weight_prep_plan", "weight_prep", "weight_prep_plan", "weight_prep", "weight_prep_plan",
                          "weight_prep", "weight_prep_plan", "weight_prep", "conv_igemm_multi", "blur_fused", "--", "fused_bias_act",
                          "upfirdn2d", "weight_prep_plan", "weight_prep", "conv_igemm[b3]", "pixel_dot", "pixel_dot", "weight_sqsum_f64",
                          "demod_bwd"],
             "w_only": ["weight_sqsum", "demod", "weight_prep_plan", "weight_prep", "weight_prep_plan", "weight_prep", "weight_prep_plan",
                        "weight_prep", "weight_prep_plan", "weight_prep", "conv_igemm_multi", "blur_fused", "--", "fused_bias_act",
                        "upfirdn2d", "pixel_dot", "weight_sqsum_f64", "demod_bwd", "conv_wgrad", "demod_wgrad"],
             "sink": ["weight_sqsum", "demod", "weight_prep_plan", "weight_prep", "weight_prep_plan", "weight_prep", "weight_prep_plan",
                      "weight_prep", "weight_prep_plan", "weight_prep", "conv_igemm_multi", "blur_fused", "--", "fused_bias_act",
                      "upfirdn2d", "weight_prep_plan", "weight_prep", "conv_igemm[b3]", "pixel_dot", "pixel_dot", "weight_sqsum_f64",
                      "demod_bwd", "conv_wgrad", "demod_wgrad"]},
 "up_nodemod": {"all": ["weight_prep_plan", "weight_prep", "weight_prep_plan", "weight_prep", "weight_prep_plan", "weight_prep",
                        "weight_prep_plan", "weight_prep", "conv_igemm_multi", "upfirdn2d", "--", "upfirdn2d", "weight_prep_plan",
                        "weight_prep", "conv_igemm[b3]", "pixel_dot", "demod_bwd", "conv_wgrad"],
                "frozen_w": ["weight_prep_plan", "weight_prep", "weight_prep_plan", "weight_prep", "weight_prep_plan", "weight_prep",
                             "weight_prep_plan", "weight_prep", "conv_igemm_multi", "upfirdn2d", "--", "upfirdn2d", "weight_prep_plan",
                             "weight_prep", "conv_igemm[b3]", "pixel_dot", "demod_bwd"],
                "w_only": ["weight_prep_plan", "weight_prep", "weight_prep_plan", "weight_prep", "weight_prep_plan", "weight_prep",
                           "weight_prep_plan", "weight_prep", "conv_igemm_multi", "upfirdn2d", "--", "upfirdn2d", "conv_wgrad"],
                "sink": ["weight_prep_plan", "weight_prep", "weight_prep_plan", "weight_prep", "weight_prep_plan", "weight_prep",
                         "weight_prep_plan", "weight_prep", "conv_igemm_multi", "upfirdn2d", "--", "upfirdn2d", "weight_prep_plan",
                         "weight_prep", "conv_igemm[b3]", "pixel_dot", "demod_bwd", "conv_wgrad"]},
 "down_chain_act": {"all": ["weight_sqsum", "demod", "upfirdn2d", "conv_igemm", "--", "act_bwd_dot", "weight_prep_plan", "weight_prep",
                            "weight_prep_plan", "weight_prep", "weight_prep_plan", "weight_prep", "weight_prep_plan", "weight_prep",
                            "conv_igemm_multi", "upfirdn2d", "pixel_dot", "weight_sqsum_f64", "demod_bwd", "conv_wgrad", "demod_wgrad"],
                    "frozen_w": ["weight_sqsum", "demod", "upfirdn2d", "conv_igemm", "--", "act_bwd_dot", "weight_prep_plan", "weight_prep",
                                 "weight_prep_plan", "weight_prep", "weight_prep_plan", "weight_prep", "weight_prep_plan", "weight_prep",
                                 "conv_igemm_multi", "upfirdn2d", "pixel_dot", "weight_sqsum_f64", "demod_bwd"],
                    "w_only": ["weight_sqsum", "demod", "upfirdn2d", "conv_igemm", "--", "act_bwd_dot", "weight_sqsum_f64", "demod_bwd",
                               "conv_wgrad", "demod_wgrad"],
                    "sink": ["weight_sqsum", "demod", "upfirdn2d", "conv_igemm", "--", "act_bwd_dot", "weight_prep_plan", "weight_prep",
                             "weight_prep_plan", "weight_prep", "weight_prep_plan", "weight_prep", "weight_prep_plan", "weight_prep",
                             "conv_igemm_multi", "upfirdn2d", "pixel_dot", "weight_sqsum_f64", "demod_bwd", "conv_wgrad", "demod_wgrad"]},
 "down_chain": {"all": ["weight_sqsum", "demod", "upfirdn2d", "conv_igemm", "--", "weight_prep_plan", "weight_prep", "weight_prep_plan",
                        "weight_prep", "weight_prep_plan", "weight_prep", "weight_prep_plan", "weight_prep", "conv_igemm_multi",
                        "upfirdn2d", "pixel_dot", "pixel_dot", "weight_sqsum_f64", "demod_bwd", "conv_wgrad", "demod_wgrad"],
                "frozen_w": ["weight_sqsum", "demod", "upfirdn2d", "conv_igemm", "--", "weight_prep_plan", "weight_prep",
                             "weight_prep_plan", "weight_prep", "weight_prep_plan", "weight_prep", "weight_prep_plan", "weight_prep",
                             "conv_igemm_multi", "upfirdn2d", "pixel_dot", "pixel_dot", "weight_sqsum_f64", "demod_bwd"],
                "w_only": ["weight_sqsum", "demod", "upfirdn2d", "conv_igemm", "--", "pixel_dot", "weight_sqsum_f64", "demod_bwd",
                           "conv_wgrad", "demod_wgrad"],
                "sink": ["weight_sqsum", "demod", "upfirdn2d", "conv_igemm", "--", "weight_prep_plan", "weight_prep", "weight_prep_plan",
                         "weight_prep", "weight_prep_plan", "weight_prep", "weight_prep_plan", "weight_prep", "conv_igemm_multi",
                         "upfirdn2d", "pixel_dot", "pixel_dot", "weight_sqsum_f64", "demod_bwd", "conv_wgrad", "demod_wgrad"]},
 "down_chain_nodemod": {"all": ["upfirdn2d", "conv_igemm", "--", "weight_prep_plan", "weight_prep", "weight_prep_plan", "weight_prep",
                                "weight_prep_plan", "weight_prep", "weight_prep_plan", "weight_prep", "conv_igemm_multi", "upfirdn2d",
                                "pixel_dot", "demod_bwd", "conv_wgrad"],
                        "frozen_w": ["upfirdn2d", "conv_igemm", "--", "weight_prep_plan", "weight_prep", "weight_prep_plan", "weight_prep",
                                     "weight_prep_plan", "weight_prep", "weight_prep_plan", "weight_prep", "conv_igemm_multi", "upfirdn2d",
                                     "pixel_dot", "demod_bwd"],
                        "w_only": ["upfirdn2d", "conv_igemm", "--", "conv_wgrad"],
                        "sink": ["upfirdn2d", "conv_igemm", "--", "weight_prep_plan", "weight_prep", "weight_prep_plan", "weight_prep",
                                 "weight_prep_plan", "weight_prep", "weight_prep_plan", "weight_prep", "conv_igemm_multi", "upfirdn2d",
                                 "pixel_dot", "demod_bwd", "conv_wgrad"]},
 "down_1x1": {"all": ["weight_sqsum", "demod", "upfirdn2d", "weight_prep_plan", "weight_prep", "conv_igemm[b3]", "--", "conv_igemm",
                      "upfirdn2d", "pixel_dot", "pixel_dot", "weight_sqsum_f64", "demod_bwd", "conv_wgrad", "demod_wgrad"],
              "frozen_w": ["weight_sqsum", "demod", "upfirdn2d", "weight_prep_plan", "weight_prep", "conv_igemm[b3]", "--", "conv_igemm",
                           "upfirdn2d", "pixel_dot", "pixel_dot", "weight_sqsum_f64", "demod_bwd"],
              "w_only": ["weight_sqsum", "demod", "upfirdn2d", "weight_prep_plan", "weight_prep", "conv_igemm[b3]", "--", "pixel_dot",
                         "weight_sqsum_f64", "demod_bwd", "conv_wgrad", "demod_wgrad"],
              "sink": ["weight_sqsum", "demod", "upfirdn2d", "weight_prep_plan", "weight_prep", "conv_igemm[b3]", "--", "conv_igemm",
                       "upfirdn2d", "pixel_dot", "pixel_dot", "weight_sqsum_f64", "demod_bwd", "conv_wgrad", "demod_wgrad"]},
 "down_fused_act": {"all": ["weight_sqsum", "demod", "weight_prep_plan", "weight_prep", "b3_blur_conv_s2_mod", "--", "act_bwd_dot",
                            "weight_prep_plan", "weight_prep", "weight_prep_plan", "weight_prep", "weight_prep_plan", "weight_prep",
                            "weight_prep_plan", "weight_prep", "conv_igemm_multi", "upfirdn2d", "pixel_dot", "weight_sqsum_f64",
                            "demod_bwd", "conv_wgrad", "demod_wgrad"],
                    "frozen_w": ["weight_sqsum", "demod", "weight_prep_plan", "weight_prep", "b3_blur_conv_s2_mod", "--", "act_bwd_dot",
                                 "weight_prep_plan", "weight_prep", "weight_prep_plan", "weight_prep", "weight_prep_plan", "weight_prep",
                                 "weight_prep_plan", "weight_prep", "conv_igemm_multi", "upfirdn2d", "pixel_dot", "weight_sqsum_f64",
                                 "demod_bwd"],
                    "w_only": ["weight_sqsum", "demod", "weight_prep_plan", "weight_prep", "b3_blur_conv_s2_mod", "--", "act_bwd_dot",
                               "weight_sqsum_f64", "demod_bwd", "conv_wgrad", "demod_wgrad"],
                    "sink": ["weight_sqsum", "demod", "weight_prep_plan", "weight_prep", "b3_blur_conv_s2_mod", "--", "act_bwd_dot",
                             "weight_prep_plan", "weight_prep", "weight_prep_plan", "weight_prep", "weight_prep_plan", "weight_prep",
                             "weight_prep_plan", "weight_prep", "conv_igemm_multi", "upfirdn2d", "pixel_dot", "weight_sqsum_f64",
                             "demod_bwd", "conv_wgrad", "demod_wgrad"]}}
EXPECTED_BF16 = {"same": {"all": ["weight_sqsum", "demod", "weight_prep_plan", "weight_prep", "conv_igemm[b3]", "--", "weight_prep_plan", "weight_prep",
                  "conv_igemm[bf16]", "pixel_dot", "pixel_dot", "weight_sqsum_f64", "demod_bwd", "conv_wgrad[bf16]", "demod_wgrad"],
          "frozen_w": ["weight_sqsum", "demod", "weight_prep_plan", "weight_prep", "conv_igemm[b3]", "--", "weight_prep_plan",
                       "weight_prep", "conv_igemm[bf16]", "pixel_dot", "pixel_dot", "weight_sqsum_f64", "demod_bwd"],
          "w_only": ["weight_sqsum", "demod", "weight_prep_plan", "weight_prep", "conv_igemm[b3]", "--", "pixel_dot", "weight_sqsum_f64",
                     "demod_bwd", "conv_wgrad[bf16]", "demod_wgrad"],
          "sink": ["weight_sqsum", "demod", "weight_prep_plan", "weight_prep", "conv_igemm[b3]", "--", "weight_prep_plan", "weight_prep",
                   "conv_igemm[bf16]", "pixel_dot", "pixel_dot", "weight_sqsum_f64", "demod_bwd", "conv_wgrad[bf16]", "demod_wgrad"]},
 "up": {"all": ["weight_sqsum", "demod", "weight_prep_plan", "weight_prep", "conv_igemm[b3]", "weight_prep_plan", "weight_prep",
                "conv_igemm[b3]", "weight_prep_plan", "weight_prep", "conv_igemm[b3]", "weight_prep_plan", "weight_prep", "conv_igemm[b3]",
                "upfirdn2d", "--", "upfirdn2d", "weight_prep_plan", "weight_prep", "conv_igemm[bf16]", "pixel_dot", "pixel_dot",
                "weight_sqsum_f64", "demod_bwd", "conv_wgrad[bf16]", "demod_wgrad"],
        "frozen_w": ["weight_sqsum", "demod", "weight_prep_plan", "weight_prep", "conv_igemm[b3]", "weight_prep_plan", "weight_prep",
                     "conv_igemm[b3]", "weight_prep_plan", "weight_prep", "conv_igemm[b3]", "weight_prep_plan", "weight_prep",
                     "conv_igemm[b3]", "upfirdn2d", "--", "upfirdn2d", "weight_prep_plan", "weight_prep", "conv_igemm[bf16]", "pixel_dot",
                     "pixel_dot", "weight_sqsum_f64", "demod_bwd"],
        "w_only": ["weight_sqsum", "demod", "weight_prep_plan", "weight_prep", "conv_igemm[b3]", "weight_prep_plan", "weight_prep",
                   "conv_igemm[b3]", "weight_prep_plan", "weight_prep", "conv_igemm[b3]", "weight_prep_plan", "weight_prep",
                   "conv_igemm[b3]", "upfirdn2d", "--", "upfirdn2d", "pixel_dot", "weight_sqsum_f64", "demod_bwd", "conv_wgrad[bf16]",
                   "demod_wgrad"],
        "sink": ["weight_sqsum", "demod", "weight_prep_plan", "weight_prep", "conv_igemm[b3]", "weight_prep_plan", "weight_prep",
                 "conv_igemm[b3]", "weight_prep_plan", "weight_prep", "conv_igemm[b3]", "weight_prep_plan", "weight_prep", "conv_igemm[b3]",
                 "upfirdn2d", "--", "upfirdn2d", "weight_prep_plan", "weight_prep", "conv_igemm[bf16]", "pixel_dot", "pixel_dot",
                 "weight_sqsum_f64", "demod_bwd", "conv_wgrad[bf16]", "demod_wgrad"]}}


class _Inputs:
    def __init__(self, name):
        from ideas_amd.model import ModulatedConv2d
        mode, k, (B, ci, co, H), self.demod, bias, self.min_blocks = CASES[name]
        self.mode, self.shape = mode, (B, ci, co, H)
        g = torch.Generator().manual_seed(sum((B, ci, co, H, k)))
        torch.manual_seed(sum((B, ci, co, H, k)))
        mod = ModulatedConv2d(ci, co, k, 8, demodulate=self.demod, upsample=mode == "up", downsample=mode == "down").cuda()
        self.w = mod.weight
        self.fir = mod.blur.kernel if mode != "same" else None
        self.x = torch.randn(B, ci, H, H, generator=g).cuda().contiguous(memory_format=CL)
        self.s = (torch.rand(B, ci, generator=g) + 0.5).cuda()
        self.b = torch.nn.Parameter((torch.randn(co, generator=g) * 0.3).cuda()) if bias else None
        self.g = g
        self.gy = None

    def leaves(self):
        return [self.x, self.s, self.w] + ([self.b] if self.b is not None else [])

    def forward(self):
        from ideas_amd.op.modulated_conv import modulated_conv2d
        y = modulated_conv2d(self.x, self.w, self.s, demodulate=self.demod, upsample=self.mode == "up", fir=self.fir,
                             act_bias=self.b, downsample=self.mode == "down")
        if self.gy is None:
            self.gy = torch.randn(y.shape, generator=self.g).to(y.dtype).cuda().contiguous(memory_format=CL)
        return y


def _node(y):
    """The modulated conv's node: ``y.grad_fn``, or behind the unfused blur / activation nodes that follow it."""
    fn = y.grad_fn
    while not type(fn).__name__.startswith("_ModConv"):
        fn = fn.next_functions[0][0]
    return fn


def run(inp: _Inputs, mode: str, monkeypatch):
    """One forward and one backward with the trainable set ``mode`` -> (trace, y, {leaf name: gradient}, shapes of the 4-D tensors
    the conv's node saved)."""
    from ideas_amd.op.grad_sink import grad_sink
    names = ["x", "s", "w"] + (["b"] if inp.b is not None else [])
    train = {"all": names, "sink": names, "frozen_w": [n for n in names if n != "w"], "w_only": ["w"]}[mode]
    for n, t in zip(names, inp.leaves()):
        t.requires_grad_(n in train)
        t.grad = None
    trace = []
    with monkeypatch.context() as mp:
        if inp.min_blocks is not None:
            mp.setattr(convmod, "BLUR_CONV_MOD_MIN_BLOCKS", inp.min_blocks)
        real = _lib.check

        def recorder(rc, what):
            trace.append(what.removeprefix("ideas_"))
            real(rc, what)
        mp.setattr(_lib, "check", recorder)
        y = inp.forward()
        saved = [tuple(t.shape) for t in _node(y).saved_tensors if t.dim() == 4]
        trace.append("--")
        wanted = [t for n, t in zip(names, inp.leaves()) if n in train]
        if mode == "sink":
            params = [inp.w] + ([inp.b] if inp.b is not None else [])
            for p in params:
                p.grad = torch.zeros_like(p)
            with grad_sink(params):
                y.backward(inp.gy)
            grads = [t.grad for t in wanted]
        else:
            grads = torch.autograd.grad(y, wanted, inp.gy)
    torch.cuda.synchronize()
    return trace, y.detach(), dict(zip(train, grads)), saved


@pytest.mark.parametrize("name", list(CASES))
def test_trace_and_gradients(name, monkeypatch):
    inp = _Inputs(name)
    B, ci, co, H = inp.shape
    full = None
    for mode in MODES:
        run(inp, mode, monkeypatch)                  # (anything a process does once, such as a device query, happens here)
        trace, y, grads, saved = run(inp, mode, monkeypatch)
        print(name, mode, trace)
        assert trace == EXPECTED[name][mode], (name, mode, trace)                                   # (a)
        if full is None:
            full = grads
        for n, g in grads.items():
            e = rel_err(g, full[n])
            print(name, mode, n, e)
            assert e < GTOL, (name, mode, n, e)                                                      # (b)
        if inp.mode == "down" and "w" not in grads:                                                  # (c)
            blurred = (B, ci, H + 1, H + 1) if CASES[name][1] == 3 else (B, ci, H // 2, H // 2)
            assert blurred not in saved, (name, mode, saved)


@pytest.mark.parametrize("mode", MODES[:3])
def test_torgb_does_not_retain_its_output(mode, monkeypatch):
    """(c) for the ToRGB layer (1x1, no demodulation, no activation): nothing in its backward reads y."""
    inp = _Inputs("torgb")
    for n, t in zip("xsw", inp.leaves()):
        t.requires_grad_({"frozen_w": n != "w", "w_only": n == "w"}.get(mode, True))
    y = inp.forward()
    assert tuple(y.shape) not in [tuple(t.shape) for t in _node(y).saved_tensors if t.dim() == 4]


@pytest.mark.parametrize("name", BF16_CASES)
def test_trace_bf16(name, bf16_mode, monkeypatch):  # noqa: F811
    """The same two shapes under bf16 activations, trace only: the small-image pre-scaling path of conv_wgrad_raw."""
    inp = _Inputs(name)
    for mode in MODES:
        run(inp, mode, monkeypatch)
        trace = run(inp, mode, monkeypatch)[0]
        print(name, mode, trace)
        assert trace == EXPECTED_BF16[name][mode], (name, mode, trace)
