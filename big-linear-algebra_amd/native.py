"""ctypes binding of csrc/libbla_hip.so (the C-ABI declared in include/bla.h)."""
import ctypes as C
import os

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
_SO = os.path.join(_HERE, "csrc", "libbla_hip.so")
_lib = None

ACT_NONE, ACT_RELU = 0, 1
C_F32, C_BF16 = 0, 1   # bla_gemm_bf16's c_type


class BlaError(RuntimeError):
    def __init__(self, status, msg):
        super().__init__(f"bla status {status}: {msg}")
        self.status = status


class Epilogue(C.Structure):
    """struct bla_gemm_epilogue (include/bla.h)."""
    _fields_ = [("alpha", C.c_float), ("beta", C.c_float), ("bias_row", C.c_void_p), ("bias_col", C.c_void_p),
                ("pre_act", C.c_void_p), ("ld_pre", C.c_int), ("act", C.c_int), ("relu_mask", C.c_void_p),
                ("ld_mask", C.c_int), ("row_sum_a", C.c_void_p), ("softmax_y", C.c_void_p), ("softmax_scale", C.c_float),
                ("softmax_grad", C.c_void_p), ("row_sum_alpha", C.c_float), ("row_sum_beta", C.c_float),
                ("softmax_loss_acc", C.c_void_p), ("softmax_correct_acc", C.c_void_p)]


class GemmDesc(C.Structure):
    """struct bla_gemm_desc (include/bla.h): one product of a bla_gemm_pair_f32 call."""
    _fields_ = [("transa", C.c_int), ("transb", C.c_int), ("m", C.c_int), ("n", C.c_int), ("k", C.c_int),
                ("A", C.c_void_p), ("lda", C.c_int), ("B", C.c_void_p), ("ldb", C.c_int), ("C", C.c_void_p), ("ldc", C.c_int),
                ("ep", C.POINTER(Epilogue))]


class AttentionWs(C.Structure):
    """struct bla_attention_ws (include/bla.h): six device pointers."""
    _fields_ = [(n, C.c_void_p) for n in ("q", "k", "v", "scores_raw", "weights", "attention")]


def _ptr_struct(name, fields):
    return type(name, (C.Structure,), {"_fields_": [(n, C.c_void_p) for n in fields], "__doc__": f"struct {name} of include/bla.h (device pointers)"})


class ConvBf16Map(C.Structure):
    """struct bla_conv_bf16_map (include/bla.h): a padded channel-last bf16 map [batch][hp][wp][cp] and where the tensor it carries sits in it."""
    _fields_ = [("d", C.c_void_p)] + [(n, C.c_int) for n in ("hp", "wp", "cp", "top", "left", "dilate")]


class ConvBf16Epilogue(C.Structure):
    """struct bla_conv_bf16_epilogue (include/bla.h)."""
    _fields_ = [("bias", C.c_void_p), ("bias_stride", C.c_int), ("relu", C.c_int), ("gate", ConvBf16Map), ("out_f32", C.c_void_p), ("dst", ConvBf16Map)]


ResnetParams = _ptr_struct("bla_resnet_params", ("conv1", "conv2", "time_w", "time_b", "res"))
ResnetGrads = _ptr_struct("bla_resnet_grads", ("conv1", "conv2", "time_w", "time_b", "res"))
ResnetWs = _ptr_struct("bla_resnet_ws", ("mu1", "sd1", "relu1", "c1", "tdense", "mu2", "sd2", "relu2", "dp", "c2", "res"))
ResnetScratch = _ptr_struct("bla_resnet_scratch", ("g_out_a", "g_out_b", "g_in", "flip"))
ResnetBf16Maps = _ptr_struct("bla_resnet_bf16_maps", ("p1", "p2", "q1"))

_VP, _I, _F, _SZ, _U64 = C.c_void_p, C.c_int, C.c_float, C.c_size_t, C.c_ulonglong
# name -> (restype, argtypes); every symbol include/bla.h declares must appear here (tests check both ways)
SIGNATURES = {
    "bla_init": (_I, [_I]), "bla_shutdown": (_I, []), "bla_is_initialized": (_I, []), "bla_device_count": (_I, []),
    "bla_last_error": (C.c_char_p, []), "bla_status_string": (C.c_char_p, [_I]), "bla_version": (C.c_char_p, []),
    "bla_device_name": (_I, [C.c_char_p, _I]),
    "bla_context_create": (_I, [C.POINTER(_VP), _I]), "bla_context_set_current": (_I, [_VP]), "bla_context_destroy": (_I, [_VP]),
    "bla_malloc": (_I, [C.POINTER(_VP), _SZ]), "bla_free": (_I, [_VP]),
    "bla_memcpy_h2d": (_I, [_VP, _VP, _SZ, _VP]), "bla_memcpy_d2h": (_I, [_VP, _VP, _SZ, _VP]),
    "bla_memcpy_d2d": (_I, [_VP, _VP, _SZ, _VP]), "bla_memset": (_I, [_VP, _I, _SZ, _VP]),
    "bla_stream_sync": (_I, [_VP]), "bla_default_stream": (_VP, []),
    "bla_event_create": (_I, [C.POINTER(_VP)]), "bla_event_destroy": (_I, [_VP]), "bla_event_record": (_I, [_VP, _VP]),
    "bla_event_elapsed_ms": (_I, [_VP, _VP, C.POINTER(_F)]),
    "bla_gemm_f32": (_I, [_VP, _I, _I, _I, _I, _I, _VP, _I, _VP, _I, _VP, _I, C.POINTER(Epilogue)]),
    "bla_gemm_set_config": (_I, [_I, _I]), "bla_gemm_last_kernel": (C.c_char_p, []),
    "bla_f32_to_bf16": (_I, [_VP, _VP, _I, _VP, _I, _I, _I]), "bla_bf16_to_f32": (_I, [_VP, _VP, _I, _VP, _I, _I, _I]),
    "bla_transpose_b16": (_I, [_VP, _VP, _I, _VP, _I, _I, _I]),
    "bla_gemm_bf16": (_I, [_VP, _I, _I, _I, _I, _I, _VP, _I, _VP, _I, _VP, _I, _I, C.POINTER(Epilogue)]),
    "bla_gemm_f32_as_bf16": (_I, [_VP, _I, _I, _I, _I, _I, _VP, _I, _VP, _I, _VP, _I, C.POINTER(Epilogue)]),
    "bla_gemm_bf16_splitk_plan": (_I, [_I] * 5 + [C.POINTER(_I), C.POINTER(_I), C.POINTER(_SZ)]),
    "bla_gemm_bf16_splitk": (_I, [_VP, _I, _I, _I, _I, _I, _VP, _I, _VP, _I, _VP, _I, _I, C.POINTER(Epilogue), _I]),
    "bla_f32_to_mxfp8": (_I, [_VP, _VP, _I, _I, _I, _I, _VP, _I, _VP, _I]), "bla_mxfp8_to_f32": (_I, [_VP, _VP, _I, _VP, _I, _VP, _I, _I, _I]),
    "bla_gemm_mxfp8": (_I, [_VP, _I, _I, _I, _VP, _I, _VP, _I, _VP, _I, _VP, _I, _VP, _I, _I, C.POINTER(Epilogue)]),
    "bla_gemm_f32_as_mxfp8": (_I, [_VP, _I, _I, _I, _I, _I, _VP, _I, _VP, _I, _VP, _I, C.POINTER(Epilogue)]),
    "bla_conv2d_weight_gradient_batched_f32_as_bf16": (_I, [_VP] * 4 + [_I] * 8),
    "bla_conv2d_weight_gradient_gathered_bf16": (_I, [_VP, _VP] + [_I] * 6 + [_VP] + [_I] * 10 + [_VP, _I]),
    "bla_conv2d_backward_gathered_f32_as_bf16": (_I, [_VP] * 6 + [_I] * 8),
    "bla_conv_bf16_layout": (_I, [_I] * 5 + [C.POINTER(_I)] * 5), "bla_conv_bf16_pad": (_I, [_VP] * 3 + [_I] * 9),
    "bla_conv_bf16_prepare_kernels": (_I, [_VP] * 3 + [_I] * 4), "bla_conv2d_gathered_bf16": (_I, [_VP, _VP, _I, _VP] + [_I] * 8 + [_VP, _VP, _I]),
    "bla_conv2d_gathered_bf16_chained": (_I, [_VP, _VP, _I, _VP] + [_I] * 8 + [C.POINTER(ConvBf16Epilogue)]),
    "bla_conv2d_forward_batched_f32_as_bf16": (_I, [_VP] * 4 + [_I] * 7 + [_VP, _I]), "bla_conv2d_backward_batched_f32_as_bf16": (_I, [_VP] * 6 + [_I] * 7),
    "bla_scale_f32": (_I, [_VP, _VP, _SZ, _F]), "bla_add_f32": (_I, [_VP, _VP, _VP, _SZ]),
    "bla_hadamard_f32": (_I, [_VP, _VP, _VP, _SZ]), "bla_axpy_f32": (_I, [_VP, _VP, _VP, _F, _SZ]),
    "bla_relu_f32": (_I, [_VP, _VP, _SZ]), "bla_relu_ddx_f32": (_I, [_VP, _VP, _SZ]),
    "bla_add_tile_columns_f32": (_I, [_VP, _VP, _I, _I, _VP, _I]), "bla_add_tile_rows_f32": (_I, [_VP, _VP, _I, _I, _VP]),
    "bla_transpose_f32": (_I, [_VP, _VP, _VP, _I, _I]), "bla_row_sum_f32": (_I, [_VP, _VP, _I, _I, _VP]),
    "bla_col_sum_f32": (_I, [_VP, _VP, _I, _I, _VP, _I]), "bla_frobenius_f32": (_I, [_VP, _VP, _SZ, _VP]),
    "bla_max_f32": (_I, [_VP, _VP, _SZ, _VP]), "bla_zscore_f32": (_I, [_VP, _VP, _SZ]),
    "bla_softmax_cols_f32": (_I, [_VP, _VP, _I, _I]), "bla_softmax_rows_f32": (_I, [_VP, _VP, _I, _I]),
    "bla_softmax_cols_grad_f32": (_I, [_VP, _VP, _I, _I, _VP, _F, _VP]),
    "bla_gemm_f64": (_I, [_VP, _I, _I, _I, _I, _I, _VP, _I, _VP, _I, _VP, _I, C.c_double, C.c_double]),
    "bla_scale_f64": (_I, [_VP, _VP, _SZ, C.c_double]), "bla_add_f64": (_I, [_VP, _VP, _VP, _SZ]), "bla_hadamard_f64": (_I, [_VP, _VP, _VP, _SZ]),
    "bla_add_tile_columns_f64": (_I, [_VP, _VP, _I, _I, _VP, _I]), "bla_add_tile_rows_f64": (_I, [_VP, _VP, _I, _I, _VP]),
    "bla_transpose_f64": (_I, [_VP, _VP, _VP, _I, _I]), "bla_row_sum_f64": (_I, [_VP, _VP, _I, _I, _VP]), "bla_col_sum_f64": (_I, [_VP, _VP, _I, _I, _VP, _I]),
    "bla_frobenius_f64": (_I, [_VP, _VP, _SZ, _VP]), "bla_max_f64": (_I, [_VP, _VP, _SZ, _VP]), "bla_zscore_f64": (_I, [_VP, _VP, _SZ]),
    "bla_im2col_f64": (_I, [_VP, _VP, _VP] + [_I] * 5), "bla_col2im_f64": (_I, [_VP, _VP, _VP] + [_I] * 5),
    "bla_kernels_to_matrix_f64": (_I, [_VP, _VP, _VP, _I, _I, _I]), "bla_matrix_to_kernels_f64": (_I, [_VP, _VP, _VP, _I, _I, _I]),
    "bla_reshape_channels_matrix_f64": (_I, [_VP, _VP, _VP, _I, _I]), "bla_reshape_matrix_channels_f64": (_I, [_VP, _VP, _VP, _I, _I]),
    "bla_conv_forward_f64": (_I, [_VP] * 7 + [_I] * 6), "bla_conv_backward_f64": (_I, [_VP] * 9 + [_I] * 6),
    "bla_group_norm_f64": (_I, [_VP] * 5 + [_I] * 3), "bla_group_norm_ddx_f64": (_I, [_VP] * 6 + [_I] * 3),
    "bla_relu_f64": (_I, [_VP, _VP, _SZ]), "bla_softmax_cols_f64": (_I, [_VP, _VP, _I, _I]), "bla_softmax_rows_f64": (_I, [_VP, _VP, _I, _I]),
    "bla_conv_out_hw": (_I, [_I, _I, _I, C.POINTER(_I), C.POINTER(_I)]),
    "bla_im2col_f32": (_I, [_VP, _VP, _VP, _I, _I, _I, _I, _I]), "bla_col2im_f32": (_I, [_VP, _VP, _VP, _I, _I, _I, _I, _I]),
    "bla_kernels_to_matrix_f32": (_I, [_VP, _VP, _VP, _I, _I, _I]), "bla_matrix_to_kernels_f32": (_I, [_VP, _VP, _VP, _I, _I, _I]),
    "bla_reshape_channels_matrix_f32": (_I, [_VP, _VP, _VP, _I, _I]), "bla_reshape_matrix_channels_f32": (_I, [_VP, _VP, _VP, _I, _I]),
    "bla_conv_forward_f32": (_I, [_VP] * 7 + [_I] * 6), "bla_conv_backward_f32": (_I, [_VP] * 9 + [_I] * 6),
    "bla_conv2d_forward_f32": (_I, [_VP] * 4 + [_I] * 6), "bla_conv2d_backward_f32": (_I, [_VP] * 7 + [_I] * 6),
    "bla_conv2d_forward_batched_f32": (_I, [_VP] * 4 + [_I] * 7), "bla_conv2d_backward_batched_f32": (_I, [_VP] * 7 + [_I] * 7),
    "bla_conv_last_plan": (C.c_char_p, []),
    "bla_conv2d_forward_fused_f32": (_I, [_VP] * 4 + [_I] * 7 + [_VP, _I, _VP, _VP, _VP, _VP]),
    "bla_conv2d_backward_prepared_f32": (_I, [_VP] * 7 + [_I] * 7 + [_VP] * 3),
    "bla_conv_prepare_kernels_f32": (_I, [_VP, _VP, _VP, _I, _I, _I, _I]), "bla_conv_prep_mode": (_I, [_I] * 8),
    "bla_conv_padded_layout": (_I, [_I] * 4 + [C.POINTER(_I)] * 5),
    "bla_group_norm_f32": (_I, [_VP] * 5 + [_I] * 3), "bla_group_norm_ddx_f32": (_I, [_VP] * 6 + [_I] * 3),
    "bla_relu_mask_f32": (_I, [_VP, _VP, _VP, _VP, _SZ]), "bla_dropout_f32": (_I, [_VP, _VP, _VP, _VP, _SZ]),
    "bla_dropout_mask_f32": (_I, [_VP, _VP, _VP, _SZ]), "bla_nearest_neighbours_f32": (_I, [_VP, _VP, _VP] + [_I] * 6),
    "bla_nearest_neighbours_ddx_f32": (_I, [_VP, _VP, _VP] + [_I] * 6), "bla_softmax_ddx_f32": (_I, [_VP, _VP, _VP, _VP, _I, _I]),
    "bla_attention_forward_f32": (_I, [_VP] * 9 + [_I] * 3), "bla_attention_backward_f32": (_I, [_VP] * 14 + [_I] * 4),
    "bla_group_norm_relu_f32": (_I, [_VP] * 5 + [_I] * 3), "bla_sum_f32": (_I, [_VP, _VP, _VP, _VP, _SZ]),
    "bla_resnet_forward_f32": (_I, [_VP] * 7 + [_I] * 7), "bla_resnet_backward_f32": (_I, [_VP] * 9 + [_I] * 7),
    "bla_layer_net_create": (_I, [C.POINTER(_VP), C.POINTER(_I), _I, _I, C.POINTER(_I), C.POINTER(_F)]), "bla_layer_net_destroy": (_I, [_VP]),
    "bla_layer_net_param_count": (_SZ, [_VP]), "bla_layer_net_params": (_VP, [_VP]), "bla_layer_net_weights": (_VP, [_VP, _I]),
    "bla_layer_net_biases": (_VP, [_VP, _I]), "bla_layer_net_nodes": (_VP, [_VP, _I]), "bla_layer_net_raw_nodes": (_VP, [_VP, _I]),
    "bla_layer_net_forward_f32": (_I, [_VP, _VP, _VP]), "bla_layer_net_backward_f32": (_I, [_VP, _VP, _VP, _F]),
    "bla_unet_create_batched": (_I, [C.POINTER(_VP), _VP, _I]), "bla_unet_batch": (_I, [_VP]),
    "bla_unet_create_mixed": (_I, [C.POINTER(_VP), _VP, _I, _I]), "bla_unet_products": (_I, [_VP]),
    "bla_conv_bf16_prepare_kernels_table": (_I, [_VP, _VP, _I, _SZ]),
    "bla_unet_create": (_I, [C.POINTER(_VP), _VP]), "bla_unet_destroy": (_I, [_VP]), "bla_unet_param_count": (_SZ, [_VP]),
    "bla_unet_params": (_VP, [_VP]), "bla_unet_grads": (_VP, [_VP]), "bla_unet_output": (_VP, [_VP]), "bla_unet_tensor_count": (_I, [_VP]),
    "bla_unet_tensor_info": (_I, [_VP, _I, C.POINTER(_SZ), C.POINTER(_SZ), C.c_char_p, _I]), "bla_unet_dropout_count": (_SZ, [_VP]),
    "bla_unet_forward_f32": (_I, [_VP, _VP, _VP, _VP, _VP]), "bla_unet_backward_f32": (_I, [_VP, _VP, _VP]),
    "bla_mnist_nn_create": (_I, [C.POINTER(_VP), C.POINTER(_I), _I]), "bla_mnist_nn_destroy": (_I, [_VP]),
    "bla_mnist_nn_param_count": (_SZ, [_VP]), "bla_mnist_nn_params": (_VP, [_VP]), "bla_mnist_nn_grads": (_VP, [_VP]),
    "bla_mnist_nn_input": (_VP, [_VP]), "bla_mnist_nn_labels": (_VP, [_VP]),
    "bla_mnist_nn_use_buckets": (_I, [_VP, _VP, _VP]), "bla_mnist_nn_set_params": (_I, [_VP, _VP]),
    "bla_mnist_nn_get_params": (_I, [_VP, _VP]), "bla_mnist_nn_activation": (_I, [_VP, _I, C.POINTER(_VP), C.POINTER(_I)]),
    "bla_mnist_nn_forward_backward": (_I, [_VP, _VP, _VP, _VP, _I]), "bla_mnist_nn_apply": (_I, [_VP, _VP, _F]),
    "bla_mnist_nn_train_step": (_I, [_VP, _VP, _VP, _VP, _F, _I]), "bla_mnist_nn_graph_step": (_I, [_VP, _VP, _F, _I, _I]),
    "bla_mnist_nn_fused_step": (_I, [_VP, _VP, _VP, _VP, _F, _I]),
    "bla_mnist_nn_gather_batch": (_I, [_VP, _VP, _VP, _VP, _I, _VP]), "bla_mnist_nn_forward": (_I, [_VP, _VP, _VP, _VP]),
    "bla_mnist_nn_metrics_enable": (_I, [_VP, _I]), "bla_mnist_nn_metrics_read": (_I, [_VP, C.POINTER(C.c_double), C.POINTER(C.c_longlong), _I]),
    "bla_gemm_batched_f32": (_I, [_VP, _I, _I, _I, _I, _I, _VP, _I, C.c_long, _VP, _I, C.c_long, _VP, _I, C.c_long, _I, C.POINTER(Epilogue), C.c_long]),
    "bla_group_norm_relu_batched_f32": (_I, [_VP, _I] + [_VP] * 4 + [_I] * 3),
    "bla_group_norm_ddx_gated_batched_f32": (_I, [_VP, _I] + [_VP] * 5 + [_I] * 3 + [_VP] * 2),
    "bla_attention_forward_batched_f32": (_I, [_VP, _I] + [_VP] * 8 + [_I] * 3), "bla_attention_backward_batched_f32": (_I, [_VP, _I] + [_VP] * 14 + [_I] * 4),
    "bla_attention_bf16_applies": (_I, [_I] * 3),
    "bla_attention_forward_batched_bf16": (_I, [_VP, _I] + [_VP] * 8 + [_I] * 3), "bla_attention_backward_batched_bf16": (_I, [_VP, _I] + [_VP] * 14 + [_I] * 3),
    "bla_attention_online_bf16_applies": (_I, [_I] * 3),
    "bla_attention_forward_batched_online_bf16": (_I, [_VP, _I] + [_VP] * 8 + [_I] * 3),
    "bla_attention_backward_batched_online_bf16": (_I, [_VP, _I] + [_VP] * 14 + [_I] * 3),
    "bla_attention_online_bf16_heads_applies": (_I, [_I] * 4),
    "bla_attention_forward_batched_online_bf16_heads": (_I, [_VP, _I] + [_VP] * 8 + [_I] * 4),
    "bla_attention_backward_batched_online_bf16_heads": (_I, [_VP, _I] + [_VP] * 14 + [_I] * 4),
    "bla_attention_f32_heads_applies": (_I, [_I] * 4),
    "bla_attention_forward_batched_f32_heads": (_I, [_VP, _I] + [_VP] * 8 + [_I] * 4),
    "bla_attention_backward_batched_f32_heads": (_I, [_VP, _I] + [_VP] * 14 + [_I] * 4),
    "bla_attention_online_f32_applies": (_I, [_I] * 4),
    "bla_attention_forward_batched_online_f32": (_I, [_VP, _I] + [_VP] * 8 + [_I] * 4),
    "bla_attention_backward_batched_online_f32": (_I, [_VP, _I] + [_VP] * 14 + [_I] * 4),
    "bla_unet_create_heads": (_I, [C.POINTER(_VP), _VP, _I, _I, _I]), "bla_unet_heads": (_I, [_VP]),
    "bla_unet_create_attention": (_I, [C.POINTER(_VP), _VP, _I, _I, _I, _I]), "bla_unet_device_bytes": (C.c_size_t, [_VP]),
    "bla_unet_set_attention": (_I, [_VP, _I]), "bla_unet_attention": (_I, [_VP]),
    "bla_resnet_forward_batched_f32": (_I, [_VP, _I] + [_VP] * 6 + [_I] * 7), "bla_resnet_backward_batched_f32": (_I, [_VP, _I] + [_VP] * 9 + [_I] * 7),
    "bla_group_norm_relu_bf16_map": (_I, [_VP, _I, _VP] + [_I] * 4 + [_VP] * 4 + [C.POINTER(ConvBf16Map)]),
    "bla_group_norm_ddx_bf16_map": (_I, [_VP, _I] + [_VP] * 4 + [_I] * 4 + [_VP, C.POINTER(ConvBf16Map)]),
    "bla_resnet_forward_batched_bf16": (_I, [_VP, _I] + [_VP] * 6 + [_I] * 7 + [C.POINTER(ResnetBf16Maps)]),
    "bla_resnet_backward_batched_bf16": (_I, [_VP, _I] + [_VP] * 9 + [_I] * 7 + [C.POINTER(ResnetBf16Maps), _I]),
    "bla_gemm_pair_f32": (_I, [_VP, _VP, _VP]), "bla_gemm_group_f32": (_I, [_VP, _VP, _I]),
    "bla_diag_mfma_rate": (_I, [_VP, _I, _I, _I, _VP]),
    "bla_graph_begin": (_I, [_VP]), "bla_graph_end": (_I, [_VP, C.POINTER(_VP)]), "bla_graph_launch": (_I, [_VP, _VP]),
    "bla_graph_destroy": (_I, [_VP]),
    "bla_dp_create": (_I, [C.POINTER(_VP), _I, _I, C.c_size_t]), "bla_dp_destroy": (_I, [_VP]),
    "bla_dp_export": (_I, [_VP, _VP]), "bla_dp_connect": (_I, [_VP, _VP]),
    "bla_dp_bucket": (_VP, [_VP, _I]), "bla_dp_count": (C.c_size_t, [_VP]),
    "bla_dp_allreduce_f32": (_I, [_VP, _VP, _I, _VP, _VP, _F]), "bla_dp_status": (_I, [_VP, C.POINTER(_I)]),
    "bla_dp_rccl_unique_id": (_I, [_VP]), "bla_dp_rccl_init": (_I, [C.POINTER(_VP), _VP, _I, _I]), "bla_dp_rccl_destroy": (_I, [_VP]),
    "bla_dp_rccl_allreduce_f32": (_I, [_VP, _VP, _VP, _SZ]), "bla_mnist_nn_dp_step_rccl": (_I, [_VP, _VP, _VP, _F, _I]),
    "bla_dp_check": (_I, [_VP]), "bla_dp_resident_blocks": (_I, [_VP]),
    "bla_dp_rccl_available": (_I, []), "bla_dp_rccl_init_all": (_I, [C.POINTER(_VP), C.POINTER(_I), _I]), "bla_dp_rccl_group_begin": (_I, []),
    "bla_dp_rccl_group_end": (_I, []), "bla_rand_guard_enter": (None, []), "bla_rand_guard_leave": (None, []),
    "bla_mnist_nn_dp_step": (_I, [_VP, _VP, _VP, _F, _I]), "bla_mnist_nn_dp_step_direct": (_I, [_VP, _VP, _VP, _F, _I]),
    "bla_rand_u32": (_I, [_VP, _VP, _SZ, _U64, _U64]), "bla_rand_normal_f32": (_I, [_VP, _VP, _SZ, _F, _F, _U64, _U64]),
    "bla_rand_bernoulli_u8": (_I, [_VP, _VP, _SZ, _F, _U64, _U64]),
    "bla_rand_permutation_u32": (_I, [_VP, _VP, _VP, _SZ, _U64, _U64]),
    "bla_adam_f32": (_I, [_VP, _VP, _VP, _VP, _VP, _SZ, _F, _F, _F, _F, _F, _F, _I]), "bla_ema_f32": (_I, [_VP, _VP, _VP, _SZ, _F]),
    "bla_sumsq_accumulate_f32": (_I, [_VP, _VP, _SZ, _VP, _VP]), "bla_clip_scale_f32": (_I, [_VP, _VP, _F, _F, _VP, _VP]),
    "bla_adam_scaled_f32": (_I, [_VP, _VP, _VP, _VP, _VP, _SZ, _F, _F, _F, _F, _F, _VP, _I]),
    "bla_diffusion_noise_gather_f32": (_I, [_VP, _VP, _VP, _SZ, _VP, _I, _I, _VP, _VP, _I, _SZ, _I, _U64, _U64, _VP, _VP, _VP, _VP, _VP]),
    "bla_diffusion_create": (_I, [C.POINTER(_VP), _I, _F, _F]), "bla_diffusion_destroy": (_I, [_VP]), "bla_diffusion_steps": (_I, [_VP]),
    "bla_diffusion_schedule": (_I, [_VP, _I, C.POINTER(C.c_double), C.POINTER(C.c_double)]),
    "bla_time_embedding_f32": (_I, [_VP, _VP, _I, _I, _VP]),
    "bla_diffusion_noise_f32": (_I, [_VP, _VP, _VP, _I, _SZ, _I, _U64, _U64, _VP, _VP, _VP, _VP]),
    "bla_diffusion_step_f32": (_I, [_VP, _VP, _VP, _VP, _I, _SZ, _I, _U64, _I, _VP]),
    "bla_unet_sample_f32": (_I, [_VP, _VP, _VP, _VP, _U64]), "bla_mse_accumulate_f32": (_I, [_VP, _VP, _VP, _SZ, _VP]),
    "bla_unet_embedding_grad_f32": (_I, [_VP, _VP, _VP]),
    "bla_class_embedding_f32": (_I, [_VP, _VP, _I, _VP, _I, _I, _F, _U64, _U64, _VP, _VP]),
    "bla_class_embedding_grad_f32": (_I, [_VP, _VP, _VP, _I, _I, _I, _VP]),
    "bla_diffusion_guided_step_f32": (_I, [_VP, _VP, _VP, _VP, _VP, _VP, _F, _I, _SZ, _I, _U64, _I, _VP, _VP, _I, _VP]),
    "bla_unet_sample_guided_f32": (_I, [_VP, _VP, _VP, _VP, _VP, _I, _VP, _F, _U64]),
    "bla_diffusion_ddim_timesteps": (_I, [_VP, _I, _VP]),
    "bla_diffusion_ddim_step_f32": (_I, [_VP, _VP, _VP, _VP, _I, _SZ, _I, _I, _F, _I, _U64, _I, _VP]),
    "bla_unet_sample_ddim_f32": (_I, [_VP, _VP, _VP, _VP, _I, _F, _I, _U64]),
    "bla_diffusion_guided_ddim_step_f32": (_I, [_VP, _VP, _VP, _VP, _VP, _VP, _F, _I, _SZ, _I, _I, _F, _I, _U64, _I, _VP, _VP, _I, _VP]),
    "bla_unet_sample_guided_ddim_f32": (_I, [_VP, _VP, _VP, _VP, _VP, _I, _VP, _F, _I, _F, _I, _U64]),
    "bla_diffusion_sample_timesteps": (_I, [_VP, _I, _I, _VP]),
    "bla_diffusion_dpmpp_coefficients": (_I, [_VP, _I, _I, _I, C.POINTER(C.c_double)]),
    "bla_diffusion_dpmpp_step_f32": (_I, [_VP, _VP, _VP, _VP, _VP, _I, _SZ, _I, _I, _I, _I, _I, _VP]),
    "bla_diffusion_guided_dpmpp_step_f32": (_I, [_VP, _VP, _VP, _VP, _VP, _VP, _F, _VP, _I, _SZ, _I, _I, _I, _I, _I, _VP, _VP, _I, _VP]),
    "bla_unet_sample_dpmpp_f32": (_I, [_VP, _VP, _VP, _VP, _I, _I, _I]),
    "bla_unet_sample_guided_dpmpp_f32": (_I, [_VP, _VP, _VP, _VP, _VP, _I, _VP, _F, _I, _I, _I]),
    "bla_diffusion_noise_at_f32": (_I, [_VP, _VP, _VP, _I, _SZ, _I, _VP, _I, _U64, _U64, _VP, _VP, _VP]),
    "bla_diffusion_vlb_terms_f32": (_I, [_VP, _VP, _VP, _VP, _VP, _VP, _VP, _I, _I, _SZ, _VP, _VP]),
    "bla_diffusion_prior_kl_f32": (_I, [_VP, _VP, _VP, _I, _SZ, _VP]),
    "bla_diffusion_vlb_weights": (_I, [_VP, _I, C.POINTER(C.c_double), C.POINTER(C.c_double)]),
    "bla_diffusion_eval_timesteps": (_I, [_VP, _I, _VP]),
    "bla_unet_evaluate_f32": (_I, [_VP, _VP, _VP, _VP, _VP, _I, _U64, _U64, _VP, _I, _VP, _VP, _VP]),
    "bla_diffusion_cosine_betas": (_I, [_I, C.c_double, C.c_double, _VP]),
    "bla_diffusion_create_from_betas": (_I, [C.POINTER(_VP), _I, _VP]),
    "bla_diffusion_set_objective": (_I, [_VP, _I, C.c_double]),
    "bla_diffusion_objective": (_I, [_VP, C.POINTER(_I), C.POINTER(C.c_double)]),
    "bla_diffusion_loss_weight": (_I, [_VP, _I, C.POINTER(C.c_double)]),
    "bla_diffusion_target_f32": (_I, [_VP, _VP, _VP, _VP, _VP, _I, _I, _SZ, _VP, _VP]),
    "bla_diffusion_to_eps_f32": (_I, [_VP, _VP, _VP, _VP, _VP, _I, _I, _SZ]),
    "bla_diffusion_loss_f32": (_I, [_VP, _VP, _VP, _VP, _I, _SZ, _VP, _VP]),
    "bla_unet_backward_from_f32": (_I, [_VP, _VP, _VP]),
}


def _preload_hip_runtime():
    """One HIP runtime per process.  PyTorch-ROCm ships its own libamdhip64.so (file name without version, SONAME
    libamdhip64.so.7); libbla_hip.so asks for libamdhip64.so.7.  If we are loaded before torch, the dynamic linker
    would satisfy that from /opt/rocm and a later `import torch` would bring a SECOND runtime into the process
    (torch then reports no device, and stream handles are not interchangeable).  Loading torch's copy first makes
    our NEEDED entry resolve to it by SONAME, whichever import order the application uses.  Pure C programs
    (the drop-in host layer) never see torch and simply use the system runtime."""
    from .build import torch_lib_dir
    tl = torch_lib_dir()
    if tl:
        try:
            C.CDLL(os.path.join(tl, "libamdhip64.so"), mode=C.RTLD_GLOBAL)
        except OSError:
            pass


def lib():
    """The loaded C-ABI library.  Fails loudly when it has not been built: there is no fallback."""
    global _lib
    if _lib is None:
        if not os.path.exists(_SO):
            raise RuntimeError(f"{_SO} is missing: run __graft_entry__.build() (hipcc --offload-arch=gfx950); "
                               "this package has no CPU fallback")
        _preload_hip_runtime()
        L = C.CDLL(_SO)
        for name, (res, args) in SIGNATURES.items():
            fn = getattr(L, name)
            fn.restype, fn.argtypes = res, args
        _lib = L
    return _lib


def check(status):
    if status != 0:
        raise BlaError(status, lib().bla_last_error().decode())


def is_available():
    """True when the library is built and a HIP device is visible."""
    return os.path.exists(_SO) and lib().bla_device_count() > 0


def init(device=0):
    check(lib().bla_init(device))


def sync(stream=None):
    check(lib().bla_stream_sync(stream))


class DeviceArray:
    """A dense row-major fp32 matrix (or any shape) in HBM, owned via bla_malloc."""

    def __init__(self, shape, dtype=np.float32):
        self.shape = tuple(int(s) for s in shape)
        self.dtype = np.dtype(dtype)
        self.nbytes = int(np.prod(self.shape)) * self.dtype.itemsize
        p = C.c_void_p()
        check(lib().bla_malloc(C.byref(p), max(self.nbytes, 4)))
        self.ptr = p.value

    def __del__(self):
        try:
            if getattr(self, "ptr", None):
                lib().bla_free(self.ptr)
                self.ptr = None
        except Exception:
            pass

    @property
    def ld(self):
        return self.shape[-1]

    def copy_from(self, a, stream=None):
        a = np.ascontiguousarray(a, self.dtype)
        assert a.shape == self.shape, (a.shape, self.shape)
        check(lib().bla_memcpy_h2d(self.ptr, a.ctypes.data, self.nbytes, stream))
        sync(stream)  # pageable source must stay alive until the copy is done
        return self

    def numpy(self, stream=None):
        out = np.empty(self.shape, self.dtype)
        check(lib().bla_memcpy_d2h(out.ctypes.data, self.ptr, self.nbytes, stream))
        sync(stream)
        return out

    def fill_bytes(self, byte, stream=None):
        check(lib().bla_memset(self.ptr, byte, self.nbytes, stream))
        return self


def to_device(a, dtype=np.float32):
    a = np.asarray(a)
    return DeviceArray(a.shape, dtype).copy_from(a)


def empty(shape, dtype=np.float32):
    return DeviceArray(shape, dtype)


def zeros(shape, dtype=np.float32):
    return DeviceArray(shape, dtype).fill_bytes(0)


def _ptr(x):
    if x is None:
        return None
    return x.ptr if isinstance(x, DeviceArray) else int(x)


def gemm_desc(a, b, c, transa=False, transb=False, epilogue=None):
    """Descriptor for gemm_pair: op(A) op(B) -> C on device arrays; `epilogue` is an Epilogue (kept alive by the caller)."""
    m = a.shape[1] if transa else a.shape[0]
    k = a.shape[0] if transa else a.shape[1]
    n = b.shape[0] if transb else b.shape[1]
    return GemmDesc(int(transa), int(transb), m, n, k, a.ptr, a.ld, b.ptr, b.ld, c.ptr, c.ld,
                    C.pointer(epilogue) if epilogue is not None else None)


def gemm_pair(p, q, stream=None):
    check(lib().bla_gemm_pair_f32(stream, C.byref(p), C.byref(q)))


def gemm_group(descs, stream=None):
    """bla_gemm_group_f32 on a sequence of GemmDesc (their epilogues are kept alive by the caller)."""
    arr = (GemmDesc * max(len(descs), 1))(*descs)
    check(lib().bla_gemm_group_f32(stream, arr, len(descs)))


def gemm_batched(a, b, c, batch, m, n, k, lda, stride_a, ldb, stride_b, ldc, stride_c, transa=False, transb=False,
                 epilogue=None, stride_pre=0, stream=None):
    """bla_gemm_batched_f32: `batch` products op(A_i) op(B_i) -> C_i, set i at base + i * stride (in elements; 0 = shared operand)."""
    check(lib().bla_gemm_batched_f32(stream, int(transa), int(transb), m, n, k, _ptr(a), lda, stride_a, _ptr(b), ldb, stride_b,
                                     _ptr(c), ldc, stride_c, batch, C.byref(epilogue) if epilogue is not None else None, stride_pre))
    return c


def gemm(a, b, c, transa=False, transb=False, alpha=1.0, beta=0.0, bias_row=None, bias_col=None, pre_act=None,
         act=ACT_NONE, relu_mask=None, stream=None, m=None, n=None, k=None, lda=None, ldb=None, ldc=None,
         row_sum_a=None, softmax_y=None, softmax_scale=0.0, softmax_grad=None, row_sum_alpha=0.0, row_sum_beta=0.0,
         softmax_loss_acc=None, softmax_correct_acc=None):
    """C = epilogue(alpha * op(A) op(B)) on device arrays; shapes default to the arrays' own."""
    if m is None:
        m = a.shape[1] if transa else a.shape[0]
    if k is None:
        k = a.shape[0] if transa else a.shape[1]
    if n is None:
        n = b.shape[0] if transb else b.shape[1]
    kb = b.shape[1] if transb else b.shape[0]
    if isinstance(b, DeviceArray) and kb != k and ldb is None:
        raise BlaError(2, f"inner dimensions differ: {k} vs {kb}")
    ep = Epilogue(alpha, beta, _ptr(bias_row), _ptr(bias_col), _ptr(pre_act), pre_act.ld if pre_act is not None else 0,
                  act, _ptr(relu_mask), relu_mask.ld if relu_mask is not None else 0, _ptr(row_sum_a), _ptr(softmax_y),
                  softmax_scale, _ptr(softmax_grad), row_sum_alpha, row_sum_beta, _ptr(softmax_loss_acc), _ptr(softmax_correct_acc))
    check(lib().bla_gemm_f32(stream, int(transa), int(transb), m, n, k, _ptr(a), lda or a.ld, _ptr(b), ldb or b.ld,
                             _ptr(c), ldc or c.ld, C.byref(ep)))
    return c


def to_bf16(a):
    """fp32 -> bf16 bit patterns (np.uint16) on the host, round to nearest even: what bla_f32_to_bf16 computes, bit for bit."""
    u = np.ascontiguousarray(a, np.float32).view(np.uint32)
    nan = (u & np.uint32(0x7FFFFFFF)) > np.uint32(0x7F800000)
    rne = (u.astype(np.uint64) + 0x7FFF + ((u >> np.uint32(16)) & np.uint32(1))) >> np.uint64(16)
    return np.where(nan, (u >> np.uint32(16)) | np.uint32(0x40), rne).astype(np.uint16)


def from_bf16(h):
    """bf16 bit patterns -> fp32, the exact widening."""
    return (np.ascontiguousarray(h, np.uint16).astype(np.uint32) << np.uint32(16)).view(np.float32)


def gemm_bf16(a, b, c, transa=False, transb=False, alpha=1.0, beta=0.0, bias_row=None, bias_col=None, act=ACT_NONE, stream=None,
              m=None, n=None, k=None, lda=None, ldb=None, ldc=None):
    """C = epilogue(alpha * op(A) op(B)) with bf16 operands (np.uint16 device arrays) and fp32 accumulation; C is fp32 or bf16 by c's dtype."""
    if m is None:
        m = a.shape[1] if transa else a.shape[0]
    if k is None:
        k = a.shape[0] if transa else a.shape[1]
    if n is None:
        n = b.shape[0] if transb else b.shape[1]
    ep = Epilogue(alpha=alpha, beta=beta, bias_row=_ptr(bias_row), bias_col=_ptr(bias_col), act=act)
    c_type = C_BF16 if c.dtype == np.uint16 else C_F32
    check(lib().bla_gemm_bf16(stream, int(transa), int(transb), m, n, k, _ptr(a), lda or a.ld, _ptr(b), ldb or b.ld, _ptr(c), ldc or c.ld,
                              c_type, C.byref(ep)))
    return c


def gemm_bf16_splitk_plan(m, n, k, splits=0, cus=0):
    """(S_eff, slabs per split, partial bytes) of a fast-path m x n x k product asked to split `splits` ways (0: the automatic rule for `cus` CUs)."""
    eff, sps, nbytes = C.c_int(), C.c_int(), C.c_size_t()
    check(lib().bla_gemm_bf16_splitk_plan(m, n, k, splits, cus, C.byref(eff), C.byref(sps), C.byref(nbytes)))
    return eff.value, sps.value, nbytes.value


def gemm_bf16_splitk(a, b, c, transa=False, transb=False, alpha=1.0, beta=0.0, bias_row=None, bias_col=None, act=ACT_NONE, stream=None,
                     m=None, n=None, k=None, lda=None, ldb=None, ldc=None, splits=0):
    """gemm_bf16 with the contraction cut into `splits` ranges whose partial tiles a second kernel adds in a fixed order (0: the automatic rule)."""
    if m is None:
        m = a.shape[1] if transa else a.shape[0]
    if k is None:
        k = a.shape[0] if transa else a.shape[1]
    if n is None:
        n = b.shape[0] if transb else b.shape[1]
    ep = Epilogue(alpha=alpha, beta=beta, bias_row=_ptr(bias_row), bias_col=_ptr(bias_col), act=act)
    c_type = C_BF16 if c.dtype == np.uint16 else C_F32
    check(lib().bla_gemm_bf16_splitk(stream, int(transa), int(transb), m, n, k, _ptr(a), lda or a.ld, _ptr(b), ldb or b.ld, _ptr(c), ldc or c.ld,
                                     c_type, C.byref(ep), splits))
    return c


# ---- MXFP8 (include/bla.h: e4m3 elements, one E8M0 scale byte per 32 elements of the contraction) -------------------------------------------------------
def _mx_round_e4m3(a):
    """fp32 magnitude bits (|x| < 512) -> the e4m3 magnitude byte: round to nearest even in integer arithmetic, saturating at 448 (0x7E)."""
    a = a.astype(np.int64)
    e = a >> 23
    normal = np.minimum(((a + 0x7FFFF + ((a >> 20) & 1)) >> 20) - (120 << 3), 0x7E)
    sh = np.clip(141 - e, 21, 40)                      # a multiple of 2^-9: mantissa >> sh; sh >= 25 is below half of 2^-9
    mant = (a & 0x7FFFFF) | 0x800000
    q, rem, half = mant >> sh, mant & ((np.int64(1) << sh) - 1), np.int64(1) << (sh - 1)
    sub = np.where(sh >= 25, 0, q + ((rem > half) | ((rem == half) & ((q & 1) == 1))))
    return np.where(e >= 121, normal, sub).astype(np.uint8)


def e4m3_round(x):
    """fp32 values with |x| < 512 -> e4m3fn bytes: round to nearest even, saturating at +-448, the sign of zero kept (the element rounding of to_mxfp8)."""
    xu = np.ascontiguousarray(x, np.float32).view(np.uint32)
    return _mx_round_e4m3(xu & np.uint32(0x7FFFFFFF)) | ((xu >> np.uint32(24)) & np.uint32(0x80)).astype(np.uint8)


def to_mxfp8(a, trans=False):
    """fp32 [rows][cols] (trans: [cols][rows]) -> (elements u8 [rows][cols rounded up to 32], scales u8 [rows][ceil(cols / 32)]) on the host: what
    bla_f32_to_mxfp8 computes, bit for bit."""
    a = np.asarray(a, np.float32)
    if a.ndim == 1:
        a = a[None, :]
    if trans:
        a = a.T
    rows, cols = a.shape
    nb = -(-cols // 32)
    v = np.zeros((rows, nb * 32), np.float32)
    v[:, :cols] = a
    v = v.reshape(rows, nb, 32)
    u = v.view(np.uint32)
    amax = (u & np.uint32(0x7FFFFFFF)).max(axis=2).astype(np.int64)
    bad = amax >= 0x7F800000
    sbyte = np.where(amax == 0, 127, np.maximum((amax >> 23) - 8, 0))
    mult = ((254 - np.where(bad, 127, sbyte)) << 23).astype(np.uint32).view(np.float32)
    with np.errstate(all="ignore"):
        x = (v * mult[:, :, None]).astype(np.float32)
    el = np.where(bad[:, :, None], np.uint8(0x7F), e4m3_round(x)).astype(np.uint8)
    return el.reshape(rows, nb * 32), np.where(bad, 255, sbyte).astype(np.uint8)


def e4m3_decode(b):
    """e4m3fn bytes -> fp32 (NaN 0x7FC00000 for 0x7F / 0xFF)."""
    b = np.asarray(b, np.uint8).astype(np.uint32)
    e, m = (b >> np.uint32(3)) & np.uint32(15), b & np.uint32(7)
    mag = np.where(e > 0, (((e + np.uint32(120)) << np.uint32(23)) | (m << np.uint32(20))).view(np.float32), m.astype(np.float32) * np.float32(2.0 ** -9))
    out = (mag.astype(np.float32).view(np.uint32) | ((b & np.uint32(0x80)) << np.uint32(24)))
    return np.where((b & np.uint32(0x7F)) == 0x7F, np.uint32(0x7FC00000), out).astype(np.uint32).view(np.float32)


def e8m0_decode(s):
    """E8M0 bytes -> fp32: 2^(s - 127), the subnormal 2^-127 for s = 0, NaN for 0xFF."""
    s = np.asarray(s, np.uint8).astype(np.uint32)
    bits = np.where(s == 0, np.uint32(0x00400000), s << np.uint32(23))
    return np.where(s == 255, np.uint32(0x7FC00000), bits).astype(np.uint32).view(np.float32)


def from_mxfp8(elems, scales):
    """(elements [rows][cols], scales [rows][>= ceil(cols / 32)]) -> fp32 [rows][cols]: decode(elem) 2^(s - 127) in fp32, what bla_mxfp8_to_f32 computes."""
    elems, scales = np.asarray(elems, np.uint8), np.asarray(scales, np.uint8)
    rows, cols = elems.shape
    sc = np.repeat(scales[:, :-(-cols // 32)], 32, axis=1)[:, :cols]
    with np.errstate(all="ignore"):
        out = (e4m3_decode(elems) * e8m0_decode(sc)).astype(np.float32)
    nan = ((elems & 0x7F) == 0x7F) | (sc == 255)
    return np.where(nan, np.uint32(0x7FC00000), out.view(np.uint32)).astype(np.uint32).view(np.float32)


def f32_to_mxfp8(src, elems, scales, rows, cols, trans=False, ld_src=None, ld=None, ld_s=None, stream=None):
    """bla_f32_to_mxfp8 on device arrays (or addresses)."""
    check(lib().bla_f32_to_mxfp8(stream, _ptr(src), ld_src or src.ld, int(trans), rows, cols, _ptr(elems), ld or elems.ld, _ptr(scales), ld_s or scales.ld))
    return elems, scales


def mxfp8_to_f32(elems, scales, dst, rows, cols, ld=None, ld_s=None, ld_dst=None, stream=None):
    """bla_mxfp8_to_f32 on device arrays (or addresses)."""
    check(lib().bla_mxfp8_to_f32(stream, _ptr(elems), ld or elems.ld, _ptr(scales), ld_s or scales.ld, _ptr(dst), ld_dst or dst.ld, rows, cols))
    return dst


def gemm_mxfp8(a, sa, b, sb, c, alpha=1.0, beta=0.0, bias_row=None, bias_col=None, act=ACT_NONE, stream=None, m=None, n=None, k=None,
               lda=None, ldsa=None, ldb=None, ldsb=None, ldc=None, c_type=None, epilogue=None):
    """C = epilogue(alpha * A B^T) with MXFP8 operands (np.uint8 device arrays: elements [m][k] / [n][k], scales [m][k / 32] / [n][k / 32]) and fp32
    accumulation; C is fp32 or bf16 by c's dtype (or c_type).  `epilogue` replaces the Epilogue built from the keyword fields."""
    if m is None:
        m = a.shape[0]
    if k is None:
        k = a.shape[1]
    if n is None:
        n = b.shape[0]
    ep = epilogue if epilogue is not None else Epilogue(alpha=alpha, beta=beta, bias_row=_ptr(bias_row), bias_col=_ptr(bias_col), act=act)
    if c_type is None:
        c_type = C_BF16 if c.dtype == np.uint16 else C_F32
    check(lib().bla_gemm_mxfp8(stream, m, n, k, _ptr(a), lda or a.ld, _ptr(sa), ldsa or sa.ld, _ptr(b), ldb or b.ld, _ptr(sb), ldsb or sb.ld,
                               _ptr(c), ldc or c.ld, c_type, C.byref(ep)))
    return c


def gemm_f32_as_mxfp8(a, b, c, transa=False, transb=False, alpha=1.0, beta=0.0, bias_row=None, bias_col=None, act=ACT_NONE, stream=None,
                      m=None, n=None, k=None, lda=None, ldb=None, ldc=None, epilogue=None):
    """bla_gemm_f32's arguments, fp32 in memory, multiplied in MXFP8: both operands quantised into the workspace, then gemm_mxfp8."""
    if m is None:
        m = a.shape[1] if transa else a.shape[0]
    if k is None:
        k = a.shape[0] if transa else a.shape[1]
    if n is None:
        n = b.shape[0] if transb else b.shape[1]
    ep = epilogue if epilogue is not None else Epilogue(alpha=alpha, beta=beta, bias_row=_ptr(bias_row), bias_col=_ptr(bias_col), act=act)
    check(lib().bla_gemm_f32_as_mxfp8(stream, int(transa), int(transb), m, n, k, _ptr(a), lda or a.ld, _ptr(b), ldb or b.ld, _ptr(c), ldc or c.ld, C.byref(ep)))
    return c


# ---- mixed-precision convolution (include/bla.h: bf16 operands, fp32 accumulation) ---------------------------------------------------------------------
def conv_bf16_layout(h, w, k, stride, data_gradient=False):
    """(hp, wp, top, left, dilate) of the padded channel-last operand: the forward input, or (data_gradient) del_y dilated by the stride."""
    v = [C.c_int() for _ in range(5)]
    check(lib().bla_conv_bf16_layout(h, w, k, stride, int(data_gradient), *[C.byref(x) for x in v]))
    return tuple(x.value for x in v)


def conv_bf16_pad(src, dst, batch, c, h, w, hp, wp, top, left, dilate=1, stream=None):
    """fp32 [batch][c][h][w] -> bf16 [batch][hp][wp][Cp] (np.uint16 device array), every element of dst written."""
    check(lib().bla_conv_bf16_pad(stream, _ptr(src), _ptr(dst), batch, c, h, w, hp, wp, top, left, dilate))
    return dst


def conv_bf16_prepare_kernels(kern, dst, f_n, c_n, k, data_gradient=False, stream=None):
    """fp32 [f_n][c_n][k][k] -> the tap-major bf16 matrix: forward [f_n][k*k*Cp], or (data_gradient) flipped and transposed [c_n][k*k*Fp]."""
    check(lib().bla_conv_bf16_prepare_kernels(stream, _ptr(kern), _ptr(dst), f_n, c_n, k, int(data_gradient)))
    return dst


class ConvBf16PrepJob(C.Structure):
    """struct bla_conv_bf16_prep_job (include/bla.h): one kernel tensor of a bla_conv_bf16_prepare_kernels_table launch."""
    _fields_ = [("kern", C.c_void_p), ("dst", C.c_void_p), ("f_n", C.c_int), ("c_n", C.c_int), ("k", C.c_int), ("data_gradient", C.c_int)]


def conv_bf16_prep_chunks(f_n, c_n, k, data_gradient=False):
    """8-element chunks of one job's destination matrix (the largest of a table is the launch's max_chunks)."""
    rows, inner = (c_n, f_n) if data_gradient else (f_n, c_n)
    return rows * k * k * ((inner + 7) // 8)


def conv_bf16_prepare_kernels_table(jobs, stream=None):
    """One launch for many conv_bf16_prepare_kernels calls: jobs = [(kern, dst, f_n, c_n, k, data_gradient), ...] on device arrays (or addresses).  The table is
    uploaded here; the fields are the caller's responsibility (include/bla.h).  Returns the device table (keep it until the stream has passed the launch)."""
    arr = (ConvBf16PrepJob * max(len(jobs), 1))(*[ConvBf16PrepJob(_ptr(kn), _ptr(d), f, c, k, int(dg)) for kn, d, f, c, k, dg in jobs])
    table = DeviceArray((max(len(jobs), 1) * C.sizeof(ConvBf16PrepJob),), np.uint8)
    check(lib().bla_memcpy_h2d(table.ptr, C.addressof(arr), len(jobs) * C.sizeof(ConvBf16PrepJob), stream))
    sync(stream)
    check(lib().bla_conv_bf16_prepare_kernels_table(stream, table.ptr, len(jobs), max([conv_bf16_prep_chunks(f, c, k, dg) for _, _, f, c, k, dg in jobs], default=0)))
    return table


UNET_PRODUCTS_F32, UNET_PRODUCTS_BF16 = 0, 1


def unet_create_mixed(cfg, batch=1, products=UNET_PRODUCTS_F32):
    """bla_unet_create_mixed: cfg is a ctypes struct bla_unet_config; returns the model handle (a c_void_p) for the bla_unet_* entries of lib()."""
    h = C.c_void_p()
    check(lib().bla_unet_create_mixed(C.byref(h), C.byref(cfg), batch, products))
    return h


def unet_products(model):
    return lib().bla_unet_products(model)


UNET_ATTENTION_F32, UNET_ATTENTION_BF16, UNET_ATTENTION_BF16_ONLINE = 0, 1, 3   # a bit set: bit 0 bf16 products, bit 1 the online softmax; 2 does not exist


def unet_set_attention(model, mode):
    """bla_unet_set_attention: where the model's attention blocks multiply; legal between passes."""
    check(lib().bla_unet_set_attention(model, mode))


def unet_attention(model):
    return lib().bla_unet_attention(model)


def attention_bf16_applies(c, s, d):
    """bla_attention_bf16_applies: host only, no device needed."""
    return bool(lib().bla_attention_bf16_applies(c, s, d))


def attention_ws(**arrays):
    """struct bla_attention_ws around device arrays (or addresses); fields not named stay NULL."""
    return AttentionWs(**{n: _ptr(a) for n, a in arrays.items()})


def attention_forward_batched_bf16(batch, x, wq, wk, wv, w, bias, ws, out, c, s, d, stream=None):
    """bla_attention_forward_batched_bf16: ws is an AttentionWs (q, k, v, weights, attention; scores_raw may be NULL)."""
    check(lib().bla_attention_forward_batched_bf16(stream, batch, _ptr(x), _ptr(wq), _ptr(wk), _ptr(wv), _ptr(w), _ptr(bias), C.byref(ws), _ptr(out), c, s, d))
    return out


def attention_backward_batched_bf16(batch, del_y, x, wq, wk, wv, w, fwd, grad, partials, del_wq, del_wk, del_wv, del_w, del_x, c, s, d, stream=None):
    """bla_attention_backward_batched_bf16: grad needs q, k, v only; partials is [batch][4 c d] floats of scratch."""
    check(lib().bla_attention_backward_batched_bf16(stream, batch, _ptr(del_y), _ptr(x), _ptr(wq), _ptr(wk), _ptr(wv), _ptr(w), C.byref(fwd), C.byref(grad),
                                                    _ptr(partials), _ptr(del_wq), _ptr(del_wk), _ptr(del_wv), _ptr(del_w), _ptr(del_x), c, s, d))


def attention_online_bf16_applies(c, s, d):
    """bla_attention_online_bf16_applies: host only, no device needed."""
    return bool(lib().bla_attention_online_bf16_applies(c, s, d))


def attention_forward_batched_online_bf16(batch, x, wq, wk, wv, w, bias, ws, out, c, s, d, stream=None):
    """bla_attention_forward_batched_online_bf16: ws needs q, k, v, attention and scores_raw ([batch][s] floats: the row log-sum-exp)."""
    check(lib().bla_attention_forward_batched_online_bf16(stream, batch, _ptr(x), _ptr(wq), _ptr(wk), _ptr(wv), _ptr(w), _ptr(bias), C.byref(ws), _ptr(out), c, s, d))
    return out


def attention_backward_batched_online_bf16(batch, del_y, x, wq, wk, wv, w, fwd, grad, partials, del_wq, del_wk, del_wv, del_w, del_x, c, s, d, stream=None):
    """bla_attention_backward_batched_online_bf16: grad needs q, k, v, attention (del_P) and scores_raw ([batch][s]: the row dots); partials [batch][4 c d]."""
    check(lib().bla_attention_backward_batched_online_bf16(stream, batch, _ptr(del_y), _ptr(x), _ptr(wq), _ptr(wk), _ptr(wv), _ptr(w), C.byref(fwd), C.byref(grad),
                                                           _ptr(partials), _ptr(del_wq), _ptr(del_wk), _ptr(del_wv), _ptr(del_w), _ptr(del_x), c, s, d))


def attention_online_bf16_heads_applies(c, s, heads, d):
    """bla_attention_online_bf16_heads_applies: host only, no device needed; d is the width of one head."""
    return bool(lib().bla_attention_online_bf16_heads_applies(c, s, heads, d))


def attention_forward_batched_online_bf16_heads(batch, x, wq, wk, wv, w, bias, ws, out, c, s, heads, d, stream=None):
    """bla_attention_forward_batched_online_bf16_heads: ws needs q, k, v, attention ([batch][s][heads d]) and scores_raw ([batch][heads][s])."""
    check(lib().bla_attention_forward_batched_online_bf16_heads(stream, batch, _ptr(x), _ptr(wq), _ptr(wk), _ptr(wv), _ptr(w), _ptr(bias), C.byref(ws), _ptr(out),
                                                                c, s, heads, d))
    return out


def attention_backward_batched_online_bf16_heads(batch, del_y, x, wq, wk, wv, w, fwd, grad, partials, del_wq, del_wk, del_wv, del_w, del_x, c, s, heads, d, stream=None):
    """bla_attention_backward_batched_online_bf16_heads: grad needs q, k, v, attention (del_P) and scores_raw ([batch][heads][s]); partials [batch][4 c heads d]."""
    check(lib().bla_attention_backward_batched_online_bf16_heads(stream, batch, _ptr(del_y), _ptr(x), _ptr(wq), _ptr(wk), _ptr(wv), _ptr(w), C.byref(fwd),
                                                                 C.byref(grad), _ptr(partials), _ptr(del_wq), _ptr(del_wk), _ptr(del_wv), _ptr(del_w), _ptr(del_x),
                                                                 c, s, heads, d))


def attention_f32_heads_applies(c, s, heads, d):
    """bla_attention_f32_heads_applies: host only, no device needed; d is the width of one head."""
    return bool(lib().bla_attention_f32_heads_applies(c, s, heads, d))


def attention_forward_batched_f32_heads(batch, x, wq, wk, wv, w, bias, ws, out, c, s, heads, d, stream=None):
    """bla_attention_forward_batched_f32_heads: ws needs q, k, v, attention ([batch][s][heads d]) and weights ([batch][heads][s][s])."""
    check(lib().bla_attention_forward_batched_f32_heads(stream, batch, _ptr(x), _ptr(wq), _ptr(wk), _ptr(wv), _ptr(w), _ptr(bias), C.byref(ws), _ptr(out), c, s, heads, d))
    return out


def attention_backward_batched_f32_heads(batch, del_y, x, wq, wk, wv, w, fwd, grad, partials, del_wq, del_wk, del_wv, del_w, del_x, c, s, heads, d, stream=None):
    """bla_attention_backward_batched_f32_heads: grad needs q, k, v and attention (del_P); partials [batch][c heads d]."""
    check(lib().bla_attention_backward_batched_f32_heads(stream, batch, _ptr(del_y), _ptr(x), _ptr(wq), _ptr(wk), _ptr(wv), _ptr(w), C.byref(fwd), C.byref(grad),
                                                         _ptr(partials), _ptr(del_wq), _ptr(del_wk), _ptr(del_wv), _ptr(del_w), _ptr(del_x), c, s, heads, d))


def unet_create_heads(cfg, batch=1, products=UNET_PRODUCTS_F32, heads=1):
    """bla_unet_create_heads: the U-Net with `heads` attention heads of width cfg.key_dim; returns the model handle like unet_create_mixed."""
    h = C.c_void_p()
    check(lib().bla_unet_create_heads(C.byref(h), C.byref(cfg), batch, products, heads))
    return h


def unet_heads(model):
    return lib().bla_unet_heads(model)


UNET_ATTENTION_F32_ONLINE = 4   # the online softmax in fp32 for every block with S > 64; the other blocks as under UNET_ATTENTION_F32


def attention_online_f32_applies(c, s, heads, d):
    """bla_attention_online_f32_applies: host only, no device needed; d is the width of one head."""
    return bool(lib().bla_attention_online_f32_applies(c, s, heads, d))


def attention_forward_batched_online_f32(batch, x, wq, wk, wv, w, bias, ws, out, c, s, heads, d, stream=None):
    """bla_attention_forward_batched_online_f32: ws needs q, k, v, attention ([batch][s][heads d]) and scores_raw ([batch][heads][s], the lse)."""
    check(lib().bla_attention_forward_batched_online_f32(stream, batch, _ptr(x), _ptr(wq), _ptr(wk), _ptr(wv), _ptr(w), _ptr(bias), C.byref(ws), _ptr(out), c, s, heads, d))
    return out


def attention_backward_batched_online_f32(batch, del_y, x, wq, wk, wv, w, fwd, grad, partials, del_wq, del_wk, del_wv, del_w, del_x, c, s, heads, d, stream=None):
    """bla_attention_backward_batched_online_f32: grad needs q, k, v, attention (del_P) and scores_raw ([batch][heads][s], the row dots); partials [batch][c heads d]."""
    check(lib().bla_attention_backward_batched_online_f32(stream, batch, _ptr(del_y), _ptr(x), _ptr(wq), _ptr(wk), _ptr(wv), _ptr(w), C.byref(fwd), C.byref(grad),
                                                          _ptr(partials), _ptr(del_wq), _ptr(del_wk), _ptr(del_wv), _ptr(del_w), _ptr(del_x), c, s, heads, d))


def unet_create_attention(cfg, batch=1, products=UNET_PRODUCTS_F32, heads=1, attention=UNET_ATTENTION_F32):
    """bla_unet_create_attention: the U-Net created in its attention mode; under UNET_ATTENTION_F32_ONLINE every shape has a route and a block on the
    online fp32 entries owns no S x S buffer."""
    h = C.c_void_p()
    check(lib().bla_unet_create_attention(C.byref(h), C.byref(cfg), batch, products, heads, attention))
    return h


def unet_device_bytes(model):
    """bla_unet_device_bytes: the sum of what the model allocated on the device."""
    return lib().bla_unet_device_bytes(model)


def conv2d_gathered_bf16(a, rows, p, batch, hp, wp, cp, k, stride, ho, wo, out, ep_bias=None, ep_bias_stride=0, stream=None):
    """out fp32 [batch][rows][ho][wo] = A [rows][k*k*cp] . gather(P [batch][hp][wp][cp]) (+ ep_bias[b * ep_bias_stride + row])."""
    check(lib().bla_conv2d_gathered_bf16(stream, _ptr(a), rows, _ptr(p), batch, hp, wp, cp, k, stride, ho, wo, _ptr(out), _ptr(ep_bias), ep_bias_stride))
    return out


def conv_bf16_map(d, hp, wp, cp, top, left, dilate=1):
    """struct bla_conv_bf16_map around a device array (or address) of a padded channel-last bf16 map."""
    return ConvBf16Map(_ptr(d), hp, wp, cp, top, left, dilate)


def conv2d_gathered_bf16_chained(a, rows, p, batch, hp, wp, cp, k, stride, ho, wo, dst=None, out_f32=None, ep_bias=None, ep_bias_stride=0, relu=False, gate=None,
                                 stream=None):
    """conv2d_gathered_bf16's product behind bias, relu and a ReLU-derivative gate, written channel-last in bf16 into the next product's padded map:
    dst and gate are conv_bf16_map(...) (or None), out_f32 the optional fp32 [batch][rows][ho][wo]."""
    ep = ConvBf16Epilogue(bias=_ptr(ep_bias), bias_stride=ep_bias_stride, relu=int(relu), gate=gate or ConvBf16Map(), out_f32=_ptr(out_f32), dst=dst or ConvBf16Map())
    check(lib().bla_conv2d_gathered_bf16_chained(stream, _ptr(a), rows, _ptr(p), batch, hp, wp, cp, k, stride, ho, wo, C.byref(ep)))
    return dst


def conv2d_forward_as_bf16(x, kern, out, batch, h, w, k, c_in, f_n, stride, ep_bias=None, ep_bias_stride=0, stream=None):
    """bla_conv2d_forward_batched_f32's arguments, fp32 in memory, multiplied in bf16: pad + prepare_kernels + gathered product in the workspace."""
    check(lib().bla_conv2d_forward_batched_f32_as_bf16(stream, _ptr(x), _ptr(kern), _ptr(out), batch, h, w, k, c_in, f_n, stride, _ptr(ep_bias), ep_bias_stride))
    return out


def conv2d_backward_as_bf16(del_y, x, kern, del_kern, del_x, batch, h, w, k, c_in, f_n, stride, stream=None):
    """Both gradients of the same convolution in bf16 (either output may be None): the materialised weight gradient, the gathered data gradient."""
    check(lib().bla_conv2d_backward_batched_f32_as_bf16(stream, _ptr(del_y), _ptr(x), _ptr(kern), _ptr(del_kern), _ptr(del_x), batch, h, w, k, c_in, f_n, stride))


def conv2d_weight_gradient_as_bf16(del_y, x, del_kern, batch, h, w, k, c_in, f_n, stride, splits=0, stream=None):
    """The bf16 weight gradient alone, its product K-split (splits: 0 = the automatic rule, 1 = the backward entry's own product)."""
    check(lib().bla_conv2d_weight_gradient_batched_f32_as_bf16(stream, _ptr(del_y), _ptr(x), _ptr(del_kern), batch, h, w, k, c_in, f_n, stride, splits))
    return del_kern


def conv2d_weight_gradient_gathered_bf16(q, hq, wq, fp, top, left, dilate, p, hp, wp, cp, batch, k, stride, ho, wo, f_n, c_n, del_kern, splits=0, stream=None):
    """The implicit bf16 weight gradient on the caller's padded copies: Q = del_y in the data-gradient layout, P = x in the forward layout."""
    check(lib().bla_conv2d_weight_gradient_gathered_bf16(stream, _ptr(q), hq, wq, fp, top, left, dilate, _ptr(p), hp, wp, cp, batch, k, stride, ho, wo, f_n, c_n,
                                                         _ptr(del_kern), splits))
    return del_kern


def conv2d_backward_gathered_as_bf16(del_y, x, kern, del_kern, del_x, batch, h, w, k, c_in, f_n, stride, splits=0, stream=None):
    """Both gradients in bf16 (either output may be None) with del_y padded once for both: the implicit weight gradient, the gathered data gradient."""
    check(lib().bla_conv2d_backward_gathered_f32_as_bf16(stream, _ptr(del_y), _ptr(x), _ptr(kern), _ptr(del_kern), _ptr(del_x), batch, h, w, k, c_in, f_n, stride, splits))


# ---- group norm into a bf16 map and the bf16 ResNet block (include/bla.h) -------------------------------------------------------------------
def group_norm_relu_bf16_map(x, batch, channels, group_size, h, w, stdevs, means, dst=None, out_f32=None, drop=None, stream=None):
    """Group norm + ReLU (+ dropout: drop is a uint8 device array, non-zero = dropped) of fp32 [batch][channels][h][w], written channel-last in bf16 into
    dst = conv_bf16_map(...) and / or planar in fp32 into out_f32; means / stdevs [batch][groups] are outputs."""
    m = dst or ConvBf16Map()
    check(lib().bla_group_norm_relu_bf16_map(stream, batch, _ptr(x), channels, group_size, h, w, _ptr(drop), _ptr(stdevs), _ptr(means), _ptr(out_f32), C.byref(m)))
    return dst


def group_norm_ddx_bf16_map(source, data, means, stdevs, batch, channels, group_size, h, w, dst=None, dest_f32=None, stream=None):
    """The group-norm gradient (no gate, no addend) of `source` at the forward input `data`, into dst = conv_bf16_map(...) and / or dest_f32."""
    m = dst or ConvBf16Map()
    check(lib().bla_group_norm_ddx_bf16_map(stream, batch, _ptr(source), _ptr(data), _ptr(means), _ptr(stdevs), channels, group_size, h, w, _ptr(dest_f32), C.byref(m)))
    return dst


def resnet_bf16_maps(p1, p2, q1=None):
    """struct bla_resnet_bf16_maps around three zero-filled padded channel-last bf16 device arrays."""
    return ResnetBf16Maps(_ptr(p1), _ptr(p2), _ptr(q1))


def resnet_forward_batched_bf16(x, temb, params, drop, ws, result, batch, h, w, cin, cout, k, tdim, group_size, maps, stream=None):
    """bla_resnet_forward_batched_f32's arguments (params: ResnetParams, ws: ResnetWs) with bf16 products inside; maps: resnet_bf16_maps(...)."""
    check(lib().bla_resnet_forward_batched_bf16(stream, batch, _ptr(x), _ptr(temb), C.byref(params), _ptr(drop), C.byref(ws), _ptr(result), h, w, cin, cout, k, tdim,
                                                group_size, C.byref(maps)))
    return result


def resnet_backward_batched_bf16(del_out, x, temb, params, ws, grads, scratch, dtb, del_x, batch, h, w, cin, cout, k, tdim, group_size, maps, splits=0, stream=None):
    """bla_resnet_backward_batched_f32's arguments (del_x may be None) with bf16 products inside; splits: the weight gradients' K-split (0 = automatic)."""
    check(lib().bla_resnet_backward_batched_bf16(stream, batch, _ptr(del_out), _ptr(x), _ptr(temb), C.byref(params), C.byref(ws), C.byref(grads), C.byref(scratch),
                                                 _ptr(dtb), _ptr(del_x), h, w, cin, cout, k, tdim, group_size, C.byref(maps), splits))
