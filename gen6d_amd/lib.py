"""ctypes binding of libgen6d_hip.so (include/gen6d_hip.h).  Fails loudly when the library is missing: there is no
CPU or PyTorch fallback for the kernels behind this ABI."""
import ctypes as C
import os

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(_HERE, "libgen6d_hip.so")      # (tools/ load profiling builds by assigning lib.LIB_PATH before the first call)

G6D_ERRORS = {-1: "G6D_EINVAL", -2: "G6D_ENOSPC", -3: "G6D_ELAUNCH"}


class G6dWinoSeg(C.Structure):
    """include/gen6d_hip.h: one map size of g6d_wino_conv3x3_multi."""
    _fields_ = [("in_", C.c_void_p), ("out_full", C.c_void_p), ("out_pool", C.c_void_p),
                ("N", C.c_int32), ("H", C.c_int32), ("W", C.c_int32), ("ld_in", C.c_int32), ("ld_full", C.c_int32), ("ld_pool", C.c_int32)]


class G6dConv16Seg(C.Structure):
    """include/gen6d_hip.h: one map size of g6d_conv16_direct_multi (16-bit activations)."""
    _fields_ = [("in_", C.c_void_p), ("out_full", C.c_void_p), ("out_pool", C.c_void_p),
                ("N", C.c_int32), ("D", C.c_int32), ("H", C.c_int32), ("W", C.c_int32), ("ld_in", C.c_int32), ("ld_full", C.c_int32),
                ("ld_pool", C.c_int32)]


class G6dRange16(C.Structure):
    """include/gen6d_hip.h: exponent table / range record of fp16 pair maps (the *_ex entry points)."""
    _fields_ = [("exps", C.c_void_p), ("rec", C.c_void_p), ("slot_in", C.c_int32), ("slot_out", C.c_int32)]


class G6dCorrSeg(C.Structure):
    """include/gen6d_hip.h: one map of g6d_corr2d_patch_multi."""
    _fields_ = [("in_", C.c_void_p), ("out", C.c_void_p), ("H", C.c_int32), ("W", C.c_int32), ("ld_in", C.c_int32), ("ld_out", C.c_int32),
                ("N", C.c_int32), ("reserved_", C.c_int32)]


class G6dFrame(C.Structure):
    """include/gen6d_hip.h: one source frame of g6d_frame_ingest (the table lives in device memory)."""
    _fields_ = [("plane0", C.c_void_p), ("plane1", C.c_void_p), ("pitch0", C.c_int32), ("pitch1", C.c_int32), ("width", C.c_int32),
                ("height", C.c_int32), ("format", C.c_int32), ("rotate", C.c_int32), ("matrix", C.c_int32), ("slot", C.c_int32),
                ("out_w", C.c_int32), ("out_h", C.c_int32), ("K", C.c_float * 9)]


class G6dMesh(C.Structure):
    """include/gen6d_hip.h: the lens mesh of one frame of g6d_frame_ingest_mesh (nodes None: the plain rule; the table lives in device memory)."""
    _fields_ = [("nodes", C.c_void_p), ("nx", C.c_int32), ("ny", C.c_int32), ("step_log2", C.c_int32), ("reserved", C.c_int32)]


# The header names the former reserved field samples_log2 (read by g6d_frame_ingest_area alone).  As for G6dConv.w_exp below, the binding
# keeps the field's earlier name in _fields_ and exposes the header's as a property.
G6dMesh.samples_log2 = property(lambda self: self.reserved, lambda self, v: setattr(self, "reserved", int(v)))


class G6dSink(C.Structure):
    """include/gen6d_hip.h: one destination of g6d_frame_emit (the table lives in device memory)."""
    _fields_ = [("plane0", C.c_void_p), ("plane1", C.c_void_p), ("pitch0", C.c_int32), ("pitch1", C.c_int32), ("width", C.c_int32),
                ("height", C.c_int32), ("format", C.c_int32), ("matrix", C.c_int32), ("slot", C.c_int32), ("pic_w", C.c_int32),
                ("pic_h", C.c_int32), ("thickness", C.c_int32), ("dot_radius", C.c_int32), ("line_rgb", C.c_int32), ("dot_rgb", C.c_int32),
                ("box", C.c_int32)]


class G6dConvRoute(C.Structure):
    """include/gen6d_hip.h: what g6d_conv_route reports about a G6dConv descriptor."""
    _fields_ = [("family", C.c_int32), ("bm", C.c_int32), ("bn", C.c_int32), ("mode", C.c_int32), ("math_mode", C.c_int32),
                ("splits", C.c_int32), ("split_source", C.c_int32), ("position_major", C.c_int32)]


class G6dConv16RouteSeg(C.Structure):
    _fields_ = [("tile0", C.c_int32), ("tw_log2", C.c_int32), ("tiles_x", C.c_int32), ("tpi", C.c_int32), ("segh_log2", C.c_int32),
                ("bands", C.c_int32)]


class G6dConv16Route(C.Structure):
    """include/gen6d_hip.h: what g6d_conv16_direct_route reports about a 16-bit direct launch."""
    _fields_ = [("kernel", C.c_int32), ("w_layout", C.c_int32), ("math_mode", C.c_int32), ("kd", C.c_int32), ("wm", C.c_int32),
                ("half_tile", C.c_int32), ("folded", C.c_int32), ("tiles", C.c_int32), ("nN", C.c_int32), ("blocks", C.c_int32),
                ("seg", G6dConv16RouteSeg * 4)]


class G6dWinoRouteSeg(C.Structure):
    _fields_ = [("qstart", C.c_int32), ("QH", C.c_int32), ("QW", C.c_int32)]


class G6dWinoRoute(C.Structure):
    """include/gen6d_hip.h: what g6d_wino_multi_route reports about a launch of one of the Winograd entry points (WINO_ROUTE_ENTRIES)."""
    _fields_ = [("entry", C.c_int32), ("family", C.c_int32), ("kd", C.c_int32), ("wide", C.c_int32), ("nq", C.c_int32), ("nwn", C.c_int32),
                ("grid2", C.c_int64), ("blocks", C.c_int32), ("nchunks", C.c_int32), ("splits", C.c_int32), ("chunks_per_split", C.c_int32),
                ("map_mode", C.c_int32), ("lds_bytes", C.c_int32), ("seg", G6dWinoRouteSeg * 4)]


# g6d_wino_multi_route's `entry` argument: the launch it stands for
WINO_ROUTE_ENTRIES = {"g6d_wino_conv3x3_multi": 0, "g6d_wino_conv3x3": 1, "g6d_wino16_conv3x3_multi": 2, "g6d_wino43_conv3x3_multi": 3,
                      "g6d_corr2d_wino_multi": 4, "g6d_corr2d_wino43_multi": 5}


class G6dConv(C.Structure):
    _fields_ = [
        ("in_", C.c_void_p), ("mul", C.c_void_p), ("in_scale", C.c_void_p), ("in_shift", C.c_void_p),
        ("weight", C.c_void_p), ("bias", C.c_void_p), ("out", C.c_void_p), ("stats", C.c_void_p),
        ("workspace", C.c_void_p), ("workspace_bytes", C.c_size_t),
        ("N", C.c_int32), ("Di", C.c_int32), ("Hi", C.c_int32), ("Wi", C.c_int32), ("Cin", C.c_int32), ("ld_in", C.c_int32),
        ("Do", C.c_int32), ("Ho", C.c_int32), ("Wo", C.c_int32), ("Cout", C.c_int32), ("ld_out", C.c_int32),
        ("kd", C.c_int32), ("kh", C.c_int32), ("kw", C.c_int32),
        ("sd", C.c_int32), ("sh", C.c_int32), ("sw", C.c_int32),
        ("pd", C.c_int32), ("ph", C.c_int32), ("pw", C.c_int32),
        ("in_relu", C.c_int32), ("in_affine_per_n", C.c_int32), ("out_act", C.c_int32),
        ("stat_rows_per_group", C.c_int32), ("split_k", C.c_int32), ("math_mode", C.c_int32),
        ("weight_wino", C.c_void_p),
        ("fin_scale", C.c_void_p), ("fin_shift", C.c_void_p), ("fin_counter", C.c_void_p),
        ("fin_count", C.c_double), ("fin_eps", C.c_double), ("fin_groups", C.c_int32),
        ("in_image_mod", C.c_int32), ("mul_group_images", C.c_int32), ("reserved_", C.c_int32),      # = the header's w_exp: see __init__
        ("weight_wino16", C.c_void_p), ("weight_wino43", C.c_void_p),
    ]


# The header names the former reserved_ field w_exp (math_mode 3's filter exponent).  The binding keeps the field under its earlier
# name in _fields_ — recorded descriptors (tests/test_multi_launch_cpu.py) list the fields by name — and exposes it as `w_exp`, the name
# the package uses: G6dConv(w_exp=...) and d.w_exp read and write that field.
def _conv_init(self, *a, w_exp=0, **k):
    C.Structure.__init__(self, *a, **k)
    if w_exp:
        self.reserved_ = int(w_exp)


G6dConv.__init__ = _conv_init
G6dConv.w_exp = property(lambda self: self.reserved_, lambda self, v: setattr(self, "reserved_", int(v)))

_P, _I, _F, _D = C.c_void_p, C.c_int, C.c_float, C.c_double

# name -> argtypes (every function returns int); mirrors include/gen6d_hip.h
SIGNATURES = {
    "g6d_marker": [_I, _P],
    "g6d_conv_igemm": [C.POINTER(G6dConv), _P],
    "g6d_conv_igemm_ex": [C.POINTER(G6dConv), _P, _P],
    "g6d_conv_plan": [C.POINTER(G6dConv)],
    "g6d_conv_route": [C.POINTER(G6dConv), C.POINTER(G6dConvRoute)],
    "g6d_corr2d_patch": [_P, _I, _I, _I, _I, _P, _I, _I, _I, _P, _I, _P, C.c_size_t, _I, _P],
    "g6d_corr2d_patch_multi": [_P, _I, _I, _P, _I, _I, _I, _P, C.c_size_t, _I, _P],
    "g6d_corr2d_wino_multi": [_P, _I, _I, _P, _I, _I, _P, C.c_size_t, _P],
    "g6d_corr2d_patch16_multi": [_P, _I, _I, _P, _I, _I, _I, _P, C.c_size_t, _I, _P],
    "g6d_stats_finalize": [_P, _I, _D, _D, _P, _P, _P],
    "g6d_affine_act_pool": [_P, _I, _P, _P, _I, _I, _I, _I, _I, _I, _I, _P, _I, _P],
    "g6d_upsample_bilinear": [_P, _I, _P, _P, _I, _I, _I, _I, _I, _I, _P, _I, _P],
    "g6d_bias_relu_pool_nchw": [_P, _P, _I, _I, _I, _I, _I, _I, _P, _P],
    "g6d_vgg_conv1_pool": [_P, _I, _I, _I, _P, _P, _I, _I, _P, _P],
    "g6d_vgg_conv1_pool_nhwc": [_P, _I, _I, _I, _P, _P, _I, _I, _P, _P],
    "g6d_vgg_conv1_pool_nhwc16": [_P, _I, _I, _I, _P, _P, _I, _I, _P, _P, _P, _I, _P],
    "g6d_conv16_direct_multi": [_P, _I, _I, _P, _I, _F, _P, _I, _I, _I, _I, _I, _I, _P, _I, _P],
    "g6d_corr16_multi": [_P, _I, _I, _P, _F, _I, _I, _I, _P],
    "g6d_product_split16": [_P, _P, _P, _P, _P, _I, _I, _I, _I, _I, _P],
    "g6d_affine_split16": [_P, _I, _P, _P, _I, _I, _I, _I, _I, _I, _I, _P, _I, _P],
    "g6d_vgg_conv1_pool_nhwc16_ex": [_P, _I, _I, _I, _P, _P, _I, _I, _P, _P, _P, _I, _P, _P],
    "g6d_conv16_direct_multi_ex": [_P, _I, _I, _P, _I, _F, _P, _I, _I, _I, _I, _I, _I, _P, _I, _P, _P],
    "g6d_corr16_multi_ex": [_P, _I, _I, _P, _F, _I, _I, _I, _P, _P],
    "g6d_product_split16_ex": [_P, _P, _P, _P, _P, _I, _I, _I, _I, _I, _P, _P],
    "g6d_affine_split16_ex": [_P, _I, _P, _P, _I, _I, _I, _I, _I, _I, _I, _P, _I, _P, _P],
    "g6d_conv16_direct_plan": [_P, _I, _I, _P, _I, _I, _I, _I, _I, _I, _P, _I],
    "g6d_conv16_direct_route": [_P, _I, _I, _P, _I, _I, _I, _I, _I, _I, _P, _I, C.POINTER(G6dConv16Route)],
    "g6d_affine_split16_to": [_P, _I, _P, _P, _I, _I, _I, _I, _I, _I, _I, _P, _I, _I, _I, _I, _P, _P],
    "g6d_upsample_bilinear_split16": [_P, _I, _P, _P, _I, _I, _I, _I, _I, _I, _P, _I, _I, _I, _I, _P, _P],
    "g6d_l2norm_split16": [_P, _I, _I, _I, _P, _I, _P, _P],
    "g6d_vgg_conv1_pool_nhwc_norm": [_P, _I, _I, _I, _P, _P, _I, _I, _P, _P, _P, _P],
    "g6d_wino_conv3x3": [_P, _I, _I, _I, _I, _I, _P, _P, _I, _I, _P, _I, _P, _I, _P, C.c_size_t, _P],
    "g6d_wino_conv3x3_multi": [_P, _I, _I, _P, _P, _I, _I, _P, C.c_size_t, _P],
    "g6d_wino16_conv3x3_multi": [_P, _I, _I, _P, _P, _I, _I, _I, _P, C.c_size_t, _P],
    "g6d_wino43_conv3x3_multi": [_P, _I, _I, _P, _P, _I, _I, _P, C.c_size_t, _P],
    "g6d_wino_multi_route": [_I, _P, _I, _I, _P, _I, _I, _I, _P, C.c_size_t, C.POINTER(G6dWinoRoute)],
    "g6d_corr2d_wino43_multi": [_P, _I, _I, _P, _I, _I, _P, C.c_size_t, _P],
    "g6d_l2norm_rows": [_P, _I, _I, _I, _P],
    "g6d_nchw_to_nhwc": [_P, _I, _I, _I, _I, _I, _P, _I, _P],
    "g6d_selector_ref_sums": [_P, _I, _I, _I, _P, _P, _P],
    "g6d_selector_prod_affine": [_P, _P, _P, _I, _I, _I, _D, _P, _P, _P],
    "g6d_selector_scan": [_P, _P, _I, _I, _I, _P, _P, _P],
    "g6d_selector_levels": [_I, _I, _P, _P, _P, _P, _P, _I, _I, _I, _D, _P, _P, _P, _P, _P],
    "g6d_refiner_volume": [_P, _P, _P, _P, _I, _I, _I, _I, _I, _I, _I, _P, _P, _P],
    "g6d_refiner_volume_kp": [_P, _P, _P, _P, _P, _P, _I, _I, _I, _I, _I, _I, _I, _P, _P, _I, _P],
    "g6d_refiner_volume_kp_pairs": [_P, _P, _P, _P, _P, _P, _I, _I, _I, _I, _I, _I, _I, _P, _P, _I, _P, _P, _P],
    "g6d_detector_assemble": [_P, _P, _P, _I, _I, _I, C.POINTER(C.c_float), _F, _I, _I, _I, _I, _P, _I, _P],
    "g6d_detector_score_mlp_max": [_P, _I, _I, _I, _P, _P, _P, _P, _P, _P],
    "g6d_detector_decode": [_P, _I, _P, _I, _P, _I, _I, _I, _I, _P, _I, _P],
    "g6d_resize_bilinear_pyramid": [_P, _I, _I, _I, _I, C.POINTER(C.c_int), C.POINTER(C.c_int), C.POINTER(C.c_void_p), _P],
    "g6d_zero_bytes": [_P, C.c_size_t, _P],
    "g6d_vps_norm": [_P, _I, _P, _I, _I, _I, _P],
    "g6d_max_an_add": [_P, _I, _I, _I, _I, _P, _P, _I, _I, _P],
    "g6d_attention": [_P, _P, _P, _I, _I, _I, _I, _P, _I, _I, _P],
    "g6d_layernorm": [_P, _I, _I, _I, _P, _P, _F, _P, _I, _P],
    "g6d_affine_act_add": [_P, _I, _P, _P, _I, _P, _I, _I, _I, _P, _I, _I, _P],
    "g6d_linear_gemv": [_P, _I, _I, _P, _P, _I, _I, _P, _P],
    "g6d_linear_gemv_batch": [_P, _I, _I, _P, _P, _I, _I, _P, _P, C.c_size_t, _P],
    "g6d_chain_crop_from_detection": [_P, _F, _P, _I, _P],
    "g6d_chain_pose_from_selection": [_P, _P, _P, _I, _P, _P, _P, _P, _P, _P, _I, _P],
    "g6d_chain_refine_prepare": [_P, _P, _P, _F, _F, _P, _P, _I, _I, _P, _P, _F, _P, _I, _P],
    "g6d_chain_refine_update": [_P, _P, _P, _P, _I, _P, _P, _I, _P],
    "g6d_warp_batch": [_P, _P, _P, _I, _I, _I, _I, _P, _P, _I, _I, _P],
    "g6d_warp_perspective": [_P, _I, _I, _I, C.POINTER(C.c_float), _P, _I, _I, _I, _F, _P],
    "g6d_track_gather": [_P, _P, _P, _P, _I, _P],
    "g6d_track_commit": [_P, _P, _P, _I, _P, _I, _F, _P, _P, _P, _P, _P, _I, _P],
    "g6d_track_gate": [_P, _P, _P, _P, _I, _P],
    "g6d_track_health": [_P, _P, _P, _P, _I, _I, _P, _I, _P, _D, _I, _D, _D, _D, _D, _D, _D, _P, _P, _P, _P, _I, _P],
    "g6d_track_verify": [_P, _P, _P, _P, _P, _D, _D, _D, _D, _I, _P, _P, _I, _P],
    "g6d_frame_ingest": [_P, _I, _P, _I, _I, _I, _P, _P],
    "g6d_sizeof_frame_desc": [],
    "g6d_frame_ingest_mesh": [_P, _P, _I, _P, _I, _I, _I, _P, _P],
    "g6d_sizeof_mesh_desc": [],
    "g6d_track_corners": [_P, _P, _P, _P, _P, _P, _I, _P],
    "g6d_frame_emit": [_P, _I, _P, _I, _I, _I, _P, _P, _P],
    "g6d_sizeof_sink_desc": [],
    "g6d_frame_emit_source": [_P, _I, _P, _I, _P, _P, _I, _I, _I, _I, _P],
    "g6d_frame_crop": [_P, _P, _P, _I, _I, _I, _P, _P, _I, _I, _P],
    "g6d_frame_ingest_area": [_P, _P, _I, _P, _I, _I, _I, _P, _P],
    "g6d_frame_crop_area": [_P, _P, _P, _I, _I, _I, _P, _P, _I, _I, _I, _P],
    "g6d_corr_fft_plan": [_P, _I, _I, _I, _I, _I, _P],
    "g6d_corr_fft_fwd": [_P, _I, _I, _I, _I, _P, _P],
    "g6d_corr_fft_gemm": [_P, _P, _P, _I, _I, _I, _I, _P],
    "g6d_corr_fft_inv": [_P, _I, _I, _I, _I, _P, _P],
}

_lib = None


def load():
    """Load (once) and type the shared library. Raises RuntimeError if it has not been built."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise RuntimeError(f"{LIB_PATH} is missing: build it with `python __graft_entry__.py` "
                           "(make -C gen6d_amd/csrc). There is no fallback path.")
    # PyTorch-ROCm ships its own HIP runtime: it has to be in the process BEFORE this library is loaded, so that both resolve to the
    # same libamdhip64 (loaded the other way round the launches here see "no ROCm-capable device")
    import torch  # noqa: F401
    lib = C.CDLL(LIB_PATH)
    for name, args in SIGNATURES.items():
        fn = getattr(lib, name)
        fn.argtypes = args
        fn.restype = C.c_int
    lib.g6d_abi_version.restype = C.c_int
    lib.g6d_sizeof_conv_desc.restype = C.c_int
    if lib.g6d_sizeof_conv_desc() != C.sizeof(G6dConv):
        raise RuntimeError("libgen6d_hip.so: G6dConv layout differs from the ctypes binding (stale build?)")
    lib.g6d_sizeof_conv_route.restype = C.c_int
    if lib.g6d_sizeof_conv_route() != C.sizeof(G6dConvRoute):
        raise RuntimeError("libgen6d_hip.so: G6dConvRoute layout differs from the ctypes binding (stale build?)")
    lib.g6d_sizeof_conv16_route.restype = C.c_int
    if lib.g6d_sizeof_conv16_route() != C.sizeof(G6dConv16Route):
        raise RuntimeError("libgen6d_hip.so: G6dConv16Route layout differs from the ctypes binding (stale build?)")
    lib.g6d_sizeof_wino_route.restype = C.c_int
    if lib.g6d_sizeof_wino_route() != C.sizeof(G6dWinoRoute):
        raise RuntimeError("libgen6d_hip.so: G6dWinoRoute layout differs from the ctypes binding (stale build?)")
    if lib.g6d_sizeof_frame_desc() != C.sizeof(G6dFrame):
        raise RuntimeError("libgen6d_hip.so: G6dFrame layout differs from the ctypes binding (stale build?)")
    if lib.g6d_sizeof_mesh_desc() != C.sizeof(G6dMesh):
        raise RuntimeError("libgen6d_hip.so: G6dMesh layout differs from the ctypes binding (stale build?)")
    if lib.g6d_sizeof_sink_desc() != C.sizeof(G6dSink):
        raise RuntimeError("libgen6d_hip.so: G6dSink layout differs from the ctypes binding (stale build?)")
    lib.g6d_last_error.restype = C.c_char_p
    lib.g6d_set_knob.argtypes, lib.g6d_set_knob.restype = [C.c_char_p, C.c_double], C.c_int
    lib.g6d_get_knob.argtypes, lib.g6d_get_knob.restype = [C.c_char_p], C.c_double
    lib.g6d_reset_knobs.argtypes, lib.g6d_reset_knobs.restype = [], None
    _lib = lib
    return lib


def set_knob(name, value):
    """Launch-policy knob of the library (include/gen6d_hip.h): tools/ and tests force kernel variants / sweep model constants with it."""
    check(load().g6d_set_knob(name.encode(), float(value)), f"g6d_set_knob({name})")


def get_knob(name):
    return load().g6d_get_knob(name.encode())


def reset_knobs():
    load().g6d_reset_knobs()


def check(rc, what):
    if rc != 0:
        msg = load().g6d_last_error().decode()
        raise RuntimeError(f"{what} failed: {G6D_ERRORS.get(rc, rc)} ({msg})")
