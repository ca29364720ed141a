"""ctypes binding of libblindno.so (the C ABI declared in include/blindno.h).

The library is loaded AFTER torch so that its HIP runtime dependency
(``libamdhip64.so.7``) resolves to the runtime torch already loaded: device
pointers and streams are then shared with PyTorch.  There is no fallback: if the
library or a GPU is missing, every op raises.
"""
from __future__ import annotations

import ctypes
import os
import threading

import torch

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("BLINDNO_LIB", os.path.join(_HERE, "libblindno.so"))

# The whole C ABI, one sub-table per header under include/ (blindno.h, then the part headers in
# the order it includes them).  An entry is its argument codes -- p pointer, i int32, l int64,
# f float, d double, s stream -- and its return type: int unless the entry ends in ">l" (int64_t)
# or ">z" (const char*).  tests/test_abi.py holds every entry to its prototype.
ABI = {
    "blindno.h": {
        "blindno_abi_version": "",
        "blindno_error_string": "i>z",
        "blindno_lift_fwd": "ppppiiiiiiis",
        "blindno_lift_bwd": "pppppiiiiiiiis",
        "blindno_project_fwd": "ppppppiiiiiiiiiis",
        "blindno_project_bwd": "pppppppiiiiiiiiiiiis",
        "blindno_rowdft": "pppiiiiiis",
        "blindno_rowdft_crop": "pppiiiiiiiis",
        "blindno_rowdft_bag_lift": "ppppppiiiiiiiiis",
        "blindno_rowdft_bag_lift_dg": "pppppppiiiiiiiiis",
        "blindno_rowidft_epi_lift": "ppppppppppiiiiiiiiis",
        "blindno_rowidft_bwd_lift": "ppppppppppiiiiiiiiis",
        "blindno_colpass": "pppppppiiiiiiiis",
        "blindno_colspec_ok": "iiiiii",
        "blindno_colspec_nchunk": "ii",
        "blindno_colspec_bwd_nchunk": "ii",
        "blindno_rowdft_cd": "ppppiiiiiiiis",
        "blindno_rowdft_bag_lift_cd": "pppppiiiiiiiis",
        "blindno_rowdft_bag_lift_cd_pack": "pppppiiiiiiiippppis",
        "blindno_colmix": "pipppiiiiiiiippps",
        "blindno_rowidft_epi_zc": "ppppppppp" + "iiiiiiiiii" + "s",
        "blindno_rowidft_epi_lift_zc": "ppppppppppppp" + "iiiiiiiiiii" + "s",
        "blindno_rowidft_bwd_zc": "pppppppppp" + "iiiiiiiii" + "s",
        "blindno_rowidft_bwd_lift_zc": "ppppppppppp" + "iiiiiiiiii" + "s",
        "blindno_rowidft_bwd_lift_zc_mix": "ppppppppppp" + "iiiiiiiiii" + "ppppi" + "s",
        "blindno_rowdft_cd_bag": "pppi" + "ppp" + "iiiiiii" + "s",
        "blindno_rowidft_bwd_zc_bag": "pppp" + "i" + "pppppppp" + "iiiiiiiii" + "s",
        "blindno_rowidft_bwd_zc_m": "p" * 13 + "i" * 13 + "s",
        "blindno_rowidft_bwd_zc_bag_m": "p" * 15 + "i" * 13 + "s",
        "blindno_colmix_u": "pippp" + "iiiiiiii" + "pppp" + "s",
        "blindno_liftgrad_rows": "iiii",
        "blindno_liftgrad_spec": "pppppppp" + "iii" + "pp" + "iiiiiii" + "pppp" + "i" + "s",
        "blindno_mix_wgrad": "ppppiiiiiis",
        "blindno_mix_wgrad_part": "pppiiiiiiis",
        "blindno_mix_wgrad_multi": "ppppis",
        "blindno_mix_wgrad_multi_u": "ppppppis",
        "blindno_mix1d": "ppppiiiiiis",
        "blindno_rowidft_epi": "ppppppiiiiiis",
        "blindno_rowidft_epi_crop": "pppppp" + "iiiiiiii" + "s",
        "blindno_rowidft_bwd": "pppppppiiiiiis",
        "blindno_rowidft_bwd_crop": "pppppppiiiiiiiis",
        "blindno_rowidft_bwd_rd": "pppppppiiiiiiiipps",
        "blindno_rowidft_epi_rd": "ppppppiiiiiippis",
        "blindno_rowidft_epi_lift_rd": "ppppppppppiiiiiiiiippis",
        "blindno_conv_wgrad": "pppiiiiiis",
        "blindno_reduce_partials": "ppiis",
        "blindno_spectrum_tile_layout": "iiiii",
        "blindno_pack_w2d": "pppiiiiis",
        "blindno_unpack_w2d": "pppiiiiis",
        "blindno_pack_w1d": "ppiiiis",
        "blindno_bagmean_fwd": "pppppiiiiis",
        "blindno_bagmean_bwd": "pppiiiiis",
        "blindno_mse": "pppplips",
        "blindno_mse_finish": "pilps",
        "blindno_mse_finish_acc": "pilpps",
        "blindno_mse_fwd": "ppplipppps",
        "blindno_rowsq": "pppiiiiiis",
        "blindno_adam": "pppplddffffs",
        "blindno_gpe_solve": "ppppddiiipppiiis",
        "blindno_trapz_rows": "ppppiis",
        # size queries (return a count, not an error code)
        "blindno_lift_bwd_nchunk": "iii",
        "blindno_conv_wgrad_nchunk": "iii",
        "blindno_rowidft_bwd_nchunk": "iiiii",
        "blindno_set_rowfuse": "i",
        "blindno_set_colfuse": "i",
        "blindno_project_bwd_nchunk": "iii",
        "blindno_project_bwd_nchunk_heads": "iii",
        "blindno_mix_wgrad_nsplit": "iiiii",
        "blindno_lift_fwd_g": "ppppiliiiiiiis",
        "blindno_lift_fwd_bag_g": "ppppiliiiiiiippppfs",
        "blindno_lift_bag_ok": "iiiiiiii",
        "blindno_lift_bwd_g": "pppppiiliiiiiiis",
        "blindno_lift_bwd_mix_g": "pppppiiliiiiiiippppiiis",
        "blindno_lift_bwd_bag_mix_g": "pppppiiliiiiiiippppiiippppffs",
        "blindno_project_fwd_g": "ppppppiliiiiiiiiiis",
        "blindno_project_bwd_g": "pppppppiiliiiiiiiiiis",
        "blindno_colpass_g": "pppppppiliiiiiiiis",
        "blindno_mix_wgrad_g": "ppppiiiiiiis",
        "blindno_rowidft_epi_g": "ppppppiliiiiiis",
        "blindno_rowidft_bwd_g": "ppppppiliiiiiis",
        "blindno_conv_wgrad_g": "pppiiiiiiis",
        "blindno_rowdft_wgrad_ok": "iiiii",
        "blindno_rowdft_wgrad_g": "pppppiippppiiiiiiiis",
        "blindno_bagmean_fwd_w": "pppppp" + "iiiii" + "s",
        "blindno_project_bwd_w": "pppppppp" + "i" + "iiiiiiiiiii" + "s",
        "blindno_project_bag_stats_floats": "iii>l",
        "blindno_project_bag_bwd_nchunk": "iii",
        "blindno_project_bag_fwd": "ppppppppp" + "iiiiiiii" + "s",
        "blindno_project_bag_bwd": "ppppppp" + "i" + "iiiiiiii" + "s",
        "blindno_pack_w2d_2": "ppppp" + "iiiii" + "s",
        "blindno_unpack_w2d_2": "ppppp" + "iiiii" + "s",
        "blindno_bn_act_nslices": "iii",
        "blindno_bn_act_fwd": "ppppppppiiiifffis",
        "blindno_bn_act_bwd": "pppppppppiiiifis",
        "blindno_gather_flat": "pppips",
        "blindno_gather_batch": "ppppipis",
        "blindno_reduce_partials_multi": "ppppis",
        "blindno_reduce_partials_pieces": "ppppppis",
        "blindno_reduce_partials_pieces_u": "pppppppppis",
        "blindno_reduce_segs_limit": "i",
        "blindno_finish_multi": "pppppppppippppis",
        "blindno_unpack_w2d_multi": "ppppis",
        "blindno_pack_w2d_multi": "ppppis",
        "blindno_fp_propagate": "pppiiiiiids",
        "blindno_bagattn_nchunk": "i",
        "blindno_bagattn_fwd": "pppppppp" + "iiii" + "s",
        "blindno_bagattn_bwd": "ppppppppppp" + "iiii" + "s",
        "blindno_conv2d_fwd": "pppp" + "iiiiiiiiiii" + "s",
        "blindno_conv2d_bwd_data": "ppp" + "iiiiiiiiiii" + "s",
        "blindno_conv2d_wgrad_nsplit": "iiiiiiiiiii",
        "blindno_conv2d_bwd_weight": "pppp" + "i" + "iiiiiiiiiii" + "s",
        "blindno_conv2d_fwd_nsplit": "iiiiiiiiiii",
        "blindno_conv2d_fwd_split": "ppppp" + "i" + "p" + "iiiiiiiiiii" + "s",
        "blindno_conv2d_bwd_data_nsplit": "iiiiiiiiiii",
        "blindno_conv2d_bwd_data_split": "pppp" + "i" + "p" + "iiiiiiiiiii" + "s",
        "blindno_conv2d_wscratch_floats": "i" + "iiiiiiiiiii",    # an int, whatever its name says
        # whole-op spectral convolutions (C hosts); int64_t byte queries
        "blindno_spectral2d_tables_bytes": "iiii>l",
        "blindno_spectral2d_tables_init": "piiii",
        "blindno_spectral_conv2d_workspace_bytes": "iiiiiiii>l",
        "blindno_spectral_conv2d_saved_bytes": "iiiii>l",
        "blindno_spectral_conv2d_fwd": "ppppppp" + "iiiiiii" + "s",
        "blindno_spectral_conv2d_bwd": "ppppppppp" + "iiiiiii" + "s",
        "blindno_spectral1d_tables_bytes": "ii>l",
        "blindno_spectral1d_tables_init": "pii",
        "blindno_spectral_conv1d_workspace_bytes": "iiiiii>l",
        "blindno_spectral_conv1d_saved_bytes": "iii>l",
        "blindno_spectral_conv1d_fwd": "pppppp" + "iiiii" + "s",
        "blindno_spectral_conv1d_bwd": "ppppppp" + "iiiii" + "s",
        # PermInvUNet_attn (csrc/unet.hip)
        "blindno_dwconv_fwd": "pppp" + "iiiiii" + "s",
        "blindno_dwconv_bwd_data": "ppp" + "iiiiii" + "s",
        "blindno_dwconv_wgrad_nsplit": "iiii",
        "blindno_dwconv_bwd_weight": "pppp" + "i" + "iiiiii" + "s",
        "blindno_cnx_pw_fwd": "ppppppppp" + "iii" + "s",
        "blindno_cnx_pw_bwd_nblk": "iii",
        "blindno_cnx_pw_bwd": "pppppppppp" + "iiii" + "s",
        "blindno_maxpool_fwd": "ppp" + "iiiii" + "s",
        "blindno_maxpool_bwd": "ppp" + "iiiii" + "s",
        "blindno_convt_fwd": "pppp" + "iiiiiiiii" + "s",
        "blindno_convt_bwd_data": "ppp" + "iiiiiiiii" + "s",
        "blindno_convt_wgrad_nparts": "iii",
        "blindno_convt_bwd_weight": "pppp" + "iiiiiiiii" + "s",
        "blindno_tok_gram_nchunk": "l",
        "blindno_tok_attn_save_floats": "iil>l",
        "blindno_tok_attn_fwd": "ppppppp" + "iil" + "f" + "s",
        "blindno_tok_attn_bwd_scratch_floats": "ii>l",
        "blindno_tok_attn_bwd": "pppppppp" + "iil" + "s",
        # DeepONet combiner + bag mean (csrc/deeponet.hip)
        "blindno_deeponet_bag_nblk": "i",
        "blindno_deeponet_bag_fwd": "pppppp" + "iiii" + "f" + "s",
        "blindno_deeponet_bag_bwd": "pppppppp" + "iiiii" + "f" + "s",
        # 3D Fourier layer (csrc/spectral3d.hip)
        "blindno_spectral3d_ok": "iiiiiiiii",
        "blindno_colpass3d": "ppppppp" + "iiiiiiiiii" + "s",
        "blindno_pack_w3d": "ppppp" + "iiiiiiii" + "s",
        "blindno_unpack_w3d": "ppppp" + "iiiiiiii" + "s",
        "blindno_lift3d_fwd": "pppp" + "iiiiiiiii" + "s",
        "blindno_lift3d_bwd_nchunk": "iiii",
        "blindno_lift3d_bwd": "ppppp" + "i" + "iiiiiiiii" + "s",
        "blindno_project3d_fwd": "pppppp" + "iiiiiiiiii" + "s",
        "blindno_project3d_bwd_nchunk": "iiii",
        "blindno_project3d_bwd": "ppppppp" + "i" + "iiiiiiiiii" + "s",
    },
    # the NIOFP3D encoder convolutions (csrc/conv3d.hip); geometry = 15 ints
    "blindno_conv3d.h": {
        "blindno_conv3d_fwd_nsplit": "i" * 15,
        "blindno_conv3d_fwd": "ppppp" + "i" + "i" * 15 + "s",
        "blindno_conv3d_bwd_data_nsplit": "i" * 15,
        "blindno_conv3d_bwd_data": "pppp" + "i" + "i" * 15 + "s",
        "blindno_conv3d_wgrad_nsplit": "i" * 15,
        "blindno_conv3d_bwd_weight": "pppp" + "i" + "i" * 15 + "s",
    },
    # the grid-resident Fokker-Planck propagator (csrc/fpe_nd.hip)
    "blindno_fpe.h": {
        "blindno_fp_propagate_nd_scratch_doubles": "iiii>l",
        "blindno_fp_propagate_nd": "pppp" + "iiiiiii" + "d" + "s",
    },
    # the grid-resident 2D GPE solver and the 2D trapezoid residual (csrc/gpe_nd.hip)
    "blindno_gpe2d.h": {
        "blindno_gpe2d_scratch_doubles": "iii>l",
        "blindno_gpe2d_launches": "ii>l",
        "blindno_gpe2d_solve": "pppp" + "ddd" + "iii" + "pipp" + "p" + "iiii" + "s",
        "blindno_trapz2_frames": "ppppp" + "iii" + "s",
    },
    # the bag-level projection of the 3D snapshot encoder (csrc/bagproj3d.hip)
    "blindno_bag3d.h": {
        "blindno_project_bag3d_stats_floats": "iiii>l",
        "blindno_project_bag3d_bwd_nchunk": "iiii",
        "blindno_project_bag3d_fwd": "ppppppppp" + "iiiiiiiiii" + "s",
        "blindno_project_bag3d_bwd": "ppppppp" + "i" + "iiiiiiiiii" + "s",
    },
    # the grid-resident 3D GPE solver and the 3D trapezoid residual (csrc/gpe_nd.hip)
    "blindno_gpe3d.h": {
        "blindno_gpe3d_scratch_doubles": "iiii>l",
        "blindno_gpe3d_launches": "ii>l",
        "blindno_gpe3d_solve": "pppp" + "dddd" + "iii" + "pipp" + "p" + "iiiii" + "s",
        "blindno_trapz3_frames": "pppppp" + "iiii" + "s",
    },
    # the record-free propagation with on-device density-error sums (csrc/fpe_nd.hip)
    "blindno_fpe_err.h": {
        "blindno_fp_error_nd_scratch_doubles": "iiii>l",
        "blindno_fp_error_nd": "pppp" + "iiiiiiii" + "d" + "s",
    },
    # the 3D GPE solver without its record, with on-device density-error sums (csrc/gpe_nd.hip)
    "blindno_gpe3d_err.h": {
        "blindno_gpe3d_error_scratch_doubles": "iiii>l",
        "blindno_gpe3d_error_launches": "iii>l",
        "blindno_gpe3d_error": "pppp" + "ppp" + "dddd" + "iiii" + "pp" + "iiiii" + "s",
    },
    # the 2D GPE solver without its record, with on-device density-error sums (csrc/gpe_nd.hip)
    "blindno_gpe2d_err.h": {
        "blindno_gpe2d_error_scratch_doubles": "iii>l",
        "blindno_gpe2d_error_launches": "iii>l",
        "blindno_gpe2d_error": "pppp" + "pp" + "ddd" + "iiii" + "pp" + "iiii" + "s",
    },
    # the bag token attention of NIOFP2D_attn in coefficient space (csrc/nioattn.hip)
    "blindno_nioattn.h": {
        "blindno_nioattn_moments_nblk": "i",
        "blindno_nioattn_moments_scratch_floats": "ii>l",
        "blindno_nioattn_moments": "pppp" + "iii" + "s",
        "blindno_nioattn_fwd": "ppppppp" + "pppp" + "iiiii" + "s",
        "blindno_nioattn_bwd_nblk": "i",
        "blindno_nioattn_bwd_scratch_floats": "iii>l",
        "blindno_nioattn_bwd": "pppppppppp" + "pppp" + "iiiiii" + "s",
    },
    # the 3D kernels of PermInvUNet_attn3D (csrc/unet3d.hip); depthwise and pool geometry =
    # (N | NC, [C,] D, H, W, KD, KH, KW), transposed conv = (N, Ci, Di, Hi, Wi, Co, Do, Ho, Wo)
    "blindno_unet3d.h": {
        "blindno_dwconv3d_fwd": "pppp" + "i" * 8 + "s",
        "blindno_dwconv3d_bwd_data": "ppp" + "i" * 8 + "s",
        "blindno_dwconv3d_wgrad_nsplit": "i" * 8,
        "blindno_dwconv3d_bwd_weight": "pppp" + "i" + "i" * 8 + "s",
        "blindno_maxpool3d_fwd": "ppp" + "i" * 7 + "s",
        "blindno_maxpool3d_bwd": "ppp" + "i" * 7 + "s",
        "blindno_convt3d_fwd": "pppp" + "i" * 9 + "s",
        "blindno_convt3d_bwd_data": "ppp" + "i" * 9 + "s",
        "blindno_convt3d_wgrad_nparts": "iiii",
        "blindno_convt3d_bwd_weight": "pppp" + "i" * 9 + "s",
    },
    # physics attention of the structured-mesh Transolver and the LayerNorm over channel planes
    # (csrc/physattn.hip); strides between snapshots are int64
    "blindno_physattn.h": {
        "blindno_physattn_ok": "iiiiii",
        "blindno_physattn_nblk": "ii",
        "blindno_physattn_fwd_scratch_floats": "iii>l",
        "blindno_physattn_fwd": "pp" + "l" + "ppppppppp" + "ppppppp" + "iii" + "s",
        "blindno_physattn_bwd_scratch_floats": "iii>l",
        "blindno_physattn_bwd": "ppp" + "l" + "ppppppp" + "ppppp" + "ppp" + "l" + "pppppppp" + "iii" + "s",
        "blindno_ln_planes_nblk": "i",
        "blindno_ln_planes_fwd": "pppppp" + "iii" + "f" + "s",
        "blindno_ln_planes_bwd": "ppppppppp" + "iii" + "s",
    },
    # the fused per-point MLP over channel planes (csrc/planemlp.hip); every activation pointer is
    # followed by its int64 stride between snapshots
    "blindno_planemlp.h": {
        "blindno_plane_mlp_ok": "iiii",
        "blindno_plane_mlp_nblk": "i",
        "blindno_plane_mlp_fwd": "pl" + "pppppp" + "pl" + "pl" + "pp" + "iiiii" + "f" + "s",
        "blindno_plane_mlp_bwd_scratch_floats": "iiiii>l",
        "blindno_plane_mlp_bwd": "pl" + "pl" + "ppppp" + "pp" + "p" + "pl" + "pppppp" + "iiiii" + "s",
    },
    # the multiplicity-weighted bag token attention of NIOFP2D_Trans_attn on a deduplicated bag
    # (csrc/bagattn_mix.hip)
    "blindno_bagattn_mix.h": {
        "blindno_bagattn_mix_ok": "iiii",
        "blindno_bagattn_mix_nchunk": "i",
        "blindno_bagattn_mix_bwd_nchunk": "i",
        "blindno_bagattn_mix_fwd_scratch_floats": "iii>l",
        "blindno_bagattn_mix_fwd": "ppppp" + "pppp" + "iiiii" + "s",
        "blindno_bagattn_mix_bwd_scratch_floats": "iii>l",
        "blindno_bagattn_mix_bwd": "ppppppp" + "ppp" + "iiiii" + "s",
    },
}

_CT = {"p": ctypes.c_void_p, "i": ctypes.c_int, "l": ctypes.c_int64, "f": ctypes.c_float,
       "d": ctypes.c_double, "s": ctypes.c_void_p}
_RET = {"": ctypes.c_int, "l": ctypes.c_int64, "z": ctypes.c_char_p}

_lock = threading.Lock()
_lib = None


class BlindnoError(RuntimeError):
    pass


def signature(name):
    """(argument codes, return code) of one entry: ("iiii", "l") for "iiii>l", ("...", "") for an
    int return.  KeyError for a name that no header's table has, or that two have."""
    found = [table[name] for table in ABI.values() if name in table]
    if len(found) != 1:
        raise KeyError(f"{name}: in {len(found)} tables of blindno._lib.ABI")
    args, _, ret = found[0].partition(">")
    return args, ret


def load():
    """Load and type the library (idempotent).  Raises BlindnoError if absent."""
    global _lib
    with _lock:
        if _lib is not None:
            return _lib
        if not os.path.exists(LIB_PATH):
            raise BlindnoError(
                f"libblindno.so not found at {LIB_PATH}; build it with "
                "`python reconstruction-of-pde-without-time-label_amd/build.py` "
                "(there is no CPU fallback)")
        lib = ctypes.CDLL(LIB_PATH)
        for table in ABI.values():
            for name, entry in table.items():
                args, _, ret = entry.partition(">")
                fn = getattr(lib, name)
                fn.argtypes = [_CT[c] for c in args]
                fn.restype = _RET[ret]
        _lib = lib
        return lib


def exported_symbols():
    return [name for table in ABI.values() for name in table]


def stream_ptr(device=None):
    return ctypes.c_void_p(torch.cuda.current_stream(device).cuda_stream)


class _TensorPtr(ctypes.c_void_p):
    """A device pointer that keeps its tensor alive: ``call(name, ptr(x.contiguous()), ...)``
    must not hand the kernel a block the caching allocator already took back (and gave to the
    next temporary in the same argument list) before the launch is enqueued."""
    __slots__ = ("tensor",)


def ptr(t):
    if t is None:
        return None
    p = _TensorPtr(t.data_ptr())
    p.tensor = t
    return p


_HOOKS = {}   # kernel name -> object with before(args) / after(args) (blindno.timing)


def query(name, *args) -> int:
    """Call a size-query entry point (returns a count)."""
    return int(getattr(load(), name)(*args))


def call(name, *args):
    lib = load()
    hook = _HOOKS.get(name)
    if hook is not None:
        hook.before(args)
    rc = getattr(lib, name)(*args)
    if hook is not None:
        hook.after(args)
    if rc != 0:
        msg = lib.blindno_error_string(rc).decode(errors="replace")
        raise BlindnoError(f"{name} failed: hip error {rc} ({msg})")
    return rc
