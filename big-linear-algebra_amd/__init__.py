"""big-linear-algebra on MI355X: hand-written gfx950 HIP kernels behind a C-ABI
(include/bla.h), a C host layer that is API-identical to the reference's
lib/matrix.h / conv.h / norm.h / util.h / layer.h, and this thin ctypes binding
used by the tests and bench.py.  There is no CPU compute path in this package:
if libbla_hip.so or a gfx950 device is missing, calls raise.
"""
from . import build as _build  # noqa: F401
from .native import (BlaError, DeviceArray, lib, init, is_available, gemm, Epilogue,  # noqa: F401
                     to_device, empty, zeros, sync, ACT_NONE, ACT_RELU, gemm_bf16, to_bf16, from_bf16, C_F32, C_BF16,
                     conv_bf16_layout, conv_bf16_pad, conv_bf16_prepare_kernels, conv2d_gathered_bf16, conv2d_forward_as_bf16,
                     conv2d_backward_as_bf16, gemm_bf16_splitk_plan, gemm_bf16_splitk, conv2d_weight_gradient_as_bf16,
                     conv2d_weight_gradient_gathered_bf16, conv2d_backward_gathered_as_bf16, conv_bf16_map,
                     conv2d_gathered_bf16_chained, group_norm_relu_bf16_map, group_norm_ddx_bf16_map, resnet_bf16_maps,
                     resnet_forward_batched_bf16, resnet_backward_batched_bf16, conv_bf16_prepare_kernels_table,
                     conv_bf16_prep_chunks, unet_create_mixed, unet_products, UNET_PRODUCTS_F32, UNET_PRODUCTS_BF16,
                     unet_set_attention, unet_attention, UNET_ATTENTION_F32, UNET_ATTENTION_BF16, attention_bf16_applies, attention_ws,
                     attention_forward_batched_bf16, attention_backward_batched_bf16, to_mxfp8, from_mxfp8, f32_to_mxfp8, mxfp8_to_f32,
                     gemm_mxfp8, gemm_f32_as_mxfp8, UNET_ATTENTION_BF16_ONLINE, attention_online_bf16_applies,
                     attention_forward_batched_online_bf16, attention_backward_batched_online_bf16, attention_online_bf16_heads_applies,
                     attention_forward_batched_online_bf16_heads, attention_backward_batched_online_bf16_heads, attention_f32_heads_applies,
                     attention_forward_batched_f32_heads, attention_backward_batched_f32_heads, unet_create_heads, unet_heads, UNET_ATTENTION_F32_ONLINE,
                     attention_online_f32_applies, attention_forward_batched_online_f32, attention_backward_batched_online_f32, unet_create_attention,
                     unet_device_bytes)

from . import native, mnist_nn  # noqa: F401,E402

build_native = _build.build_native
__all__ = ["BlaError", "DeviceArray", "lib", "init", "is_available", "gemm", "Epilogue", "to_device", "empty",
           "zeros", "sync", "build_native", "ACT_NONE", "ACT_RELU", "gemm_bf16", "to_bf16", "from_bf16", "C_F32", "C_BF16",
           "conv_bf16_layout", "conv_bf16_pad", "conv_bf16_prepare_kernels", "conv2d_gathered_bf16", "conv2d_forward_as_bf16",
           "conv2d_backward_as_bf16", "gemm_bf16_splitk_plan", "gemm_bf16_splitk", "conv2d_weight_gradient_as_bf16",
           "conv2d_weight_gradient_gathered_bf16", "conv2d_backward_gathered_as_bf16", "conv_bf16_map", "conv2d_gathered_bf16_chained",
           "group_norm_relu_bf16_map", "group_norm_ddx_bf16_map", "resnet_bf16_maps", "resnet_forward_batched_bf16", "resnet_backward_batched_bf16",
           "conv_bf16_prepare_kernels_table", "conv_bf16_prep_chunks", "unet_create_mixed", "unet_products", "UNET_PRODUCTS_F32", "UNET_PRODUCTS_BF16",
           "unet_set_attention", "unet_attention", "UNET_ATTENTION_F32", "UNET_ATTENTION_BF16", "attention_bf16_applies", "attention_ws",
           "attention_forward_batched_bf16", "attention_backward_batched_bf16", "to_mxfp8", "from_mxfp8", "f32_to_mxfp8", "mxfp8_to_f32", "gemm_mxfp8",
           "gemm_f32_as_mxfp8", "UNET_ATTENTION_BF16_ONLINE", "attention_online_bf16_applies", "attention_forward_batched_online_bf16",
           "attention_backward_batched_online_bf16", "attention_online_bf16_heads_applies", "attention_forward_batched_online_bf16_heads",
           "attention_backward_batched_online_bf16_heads", "attention_f32_heads_applies", "attention_forward_batched_f32_heads",
           "attention_backward_batched_f32_heads", "unet_create_heads", "unet_heads", "UNET_ATTENTION_F32_ONLINE", "attention_online_f32_applies",
           "attention_forward_batched_online_f32", "attention_backward_batched_online_f32", "unet_create_attention", "unet_device_bytes"]
