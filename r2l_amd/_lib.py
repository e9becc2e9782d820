"""ctypes binding of libr2l_hip.so (C ABI declared in include/r2l_hip.h).

There is deliberately NO fallback: if the shared library is missing or an export is absent the import of the
HIP path fails loudly (RuntimeError), so a GPU run can never silently route through PyTorch ops or the oracle.
"""
import ctypes
import os

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("R2L_LIB_PATH") or os.path.join(_HERE, "lib", "libr2l_hip.so")  # env override: A/B builds

_p = ctypes.c_void_p
_i = ctypes.c_int
_l = ctypes.c_int64
_f = ctypes.c_float



class Config(ctypes.Structure):
    """r2l_config of include/r2l_hip.h: explicit dispatch for the *_cfg entry points (all zero = AUTO)."""
    _fields_ = [("precision", _i), ("tiling", _i), ("coop_tiles", _i), ("reserve_cus", _i), ("dw_mode", _i),
                ("reserved", _i * 3)]


PRECISION = {"auto": 0, "fp16x2": 1, "bf16x3": 2, "fp32_mfma": 3}
TILING = {"auto": 0, "main": 1, "coop16": 3, "coopf": 4}  # (2 = "coop", the 32-ray fp32-MFMA cooperative family: retired in round 5)
DW_MODE = {"auto": 0, "fp16": 1, "exact": 2}
_cfgp = ctypes.POINTER(Config)


class TeacherFrameDesc(ctypes.Structure):
    """r2l_teacher_frame_desc of include/r2l_hip.h (r2l_teacher_frames_cfg)."""
    _fields_ = [("H", _i), ("W", _i), ("focal", _f), ("near", _f), ("far", _f), ("N_samples", _i), ("N_importance", _i),
                ("perturb", _i), ("white_bkgd", _i), ("raw_noise_std", _f), ("chunk_rays", _i), ("seed", ctypes.c_uint64),
                ("frame_id0", ctypes.c_uint64), ("ndc", _i), ("reserved", _i * 3)]


_descp = ctypes.POINTER(TeacherFrameDesc)


class TeacherStepDesc(ctypes.Structure):
    """r2l_teacher_step_desc of include/r2l_hip.h (r2l_teacher_train_step)."""
    _fields_ = [("N_rand", _i), ("N_samples", _i), ("N_importance", _i), ("perturb", _i), ("white_bkgd", _i), ("raw_noise_std", _f),
                ("near", _f), ("far", _f), ("lr", _f), ("beta1", _f), ("beta2", _f), ("eps", _f), ("step", _l),
                ("seed", ctypes.c_uint64), ("reserved", _i * 4)]


_stepp = ctypes.POINTER(TeacherStepDesc)


class StudentStepDesc(ctypes.Structure):
    """r2l_student_step_desc of include/r2l_hip.h (r2l_student_train_step)."""
    _fields_ = [("n_block", _i), ("perturb", _i), ("pack", _i), ("pool_full", _i), ("cfg", _cfgp), ("rays_per_shard", _l),
                ("n_shards", _l), ("n_draw", _l), ("draw0", _l), ("store_seed", ctypes.c_uint64), ("pool_capacity_rows", _l),
                ("pool_rows", _l), ("n_in", _l), ("n_out", _l), ("pool_key", ctypes.c_uint64), ("seed", ctypes.c_uint64),
                ("jitter_stream", ctypes.c_uint64), ("lw_rgb", ctypes.c_double), ("lr", _f), ("beta1", _f), ("beta2", _f),
                ("eps", _f), ("step", _l), ("reserved", _i * 4)]


_sstepp = ctypes.POINTER(StudentStepDesc)


class CompactStoreDesc(ctypes.Structure):
    """r2l_cstore of include/r2l_hip.h (r2l_cstore_append / r2l_cstore_batch): 72 bytes, no padding."""
    _fields_ = [("rows", _p), ("pose_c2w", _p), ("pose_focal", _p), ("shard_pose0", _p), ("capacity_shards", _l),
                ("capacity_poses", _l), ("rays_per_shard", _l), ("H", _i), ("W", _i), ("reserved", _i * 2)]


_cstorep = ctypes.POINTER(CompactStoreDesc)


class PoseRefineDesc(ctypes.Structure):
    """r2l_pose_refine_step_desc of include/r2l_hip.h (r2l_pose_refine_step)."""
    _fields_ = [("n_block", _i), ("pack", _i), ("cfg", _cfgp), ("P", _i), ("H", _i), ("W", _i), ("focal", _f), ("n", _l),
                ("seed", ctypes.c_uint64), ("iteration", _l), ("lr_rot", _f), ("lr_trans", _f), ("beta1", _f), ("beta2", _f),
                ("eps", _f), ("reserved", _i * 4)]


_posep = ctypes.POINTER(PoseRefineDesc)


class OccGridDesc(ctypes.Structure):
    """r2l_occ_grid of include/r2l_hip.h (r2l_occ_build / r2l_occ_compact): 56 bytes."""
    _fields_ = [("bits", _p), ("G", _i), ("lo", _f * 3), ("inv", _f * 3), ("step", _f * 3), ("reserved", _i * 2)]


_occp = ctypes.POINTER(OccGridDesc)


class ErtDesc(ctypes.Structure):
    """r2l_ert_desc of include/r2l_hip.h (r2l_teacher_frames_ert_cfg): 16 bytes."""
    _fields_ = [("eps", _f), ("seg", _i), ("reserved", _i * 2)]


_ertp = ctypes.POINTER(ErtDesc)


def make_config(precision="auto", tiling="auto", coop_tiles=0, reserve_cus=0, dw_mode="auto"):
    if tiling == "coop":
        raise ValueError("tiling 'coop' (the 32-ray fp32-MFMA cooperative kernels) was retired in round 5: every *_cfg call would "
                         "fail with it; 'coop16' serves those launches")
    return Config(PRECISION[precision], TILING[tiling], int(coop_tiles), int(reserve_cus), DW_MODE[dw_mode])


# name -> (restype, argtypes); one row per declaration in include/r2l_hip.h
SIGNATURES = {
    "r2l_last_error": (ctypes.c_char_p, []),
    "r2l_param_count": (_l, [_i]),
    "r2l_fwd_stream_floats": (_l, [_i]),
    "r2l_bwd_stream_floats": (_l, [_i]),
    "r2l_pack_forward": (_i, [_p, _i, _p, _p]),
    "r2l_pack_backward": (_i, [_p, _i, _p, _p]),
    "r2l_variant_for": (_i, [_l]),
    "r2l_coop_tiles_for": (_i, [_l, _i]),
    "r2l_forward_layout_for": (_i, [_l, _i]),
    "r2l_backward_layout_for": (_i, [_l]),
    "r2l_pack_forward_layout": (_i, [_p, _i, _p, _i, _p]),
    "r2l_pack_backward_layout": (_i, [_p, _i, _p, _i, _p]),
    "r2l_variant_for_cfg": (_i, [_l, _cfgp]),
    "r2l_coop_tiles_for_cfg": (_i, [_l, _i, _cfgp]),
    "r2l_forward_layout_for_cfg": (_i, [_l, _i, _cfgp]),
    "r2l_backward_layout_for_cfg": (_i, [_l, _cfgp]),
    "r2l_forward_rays": (_i, [_p, _p, _p, _p, _p, _p, _i, _p, _p, _p, _l, _p]),
    "r2l_forward_pose": (_i, [_p, _i, _i, _f, _p, _p, _p, _i, _p, _p]),
    "r2l_forward_rays_cfg": (_i, [_p, _p, _p, _p, _p, _p, _i, _p, _p, _p, _l, _p, _cfgp]),
    "r2l_forward_pose_cfg": (_i, [_p, _i, _i, _f, _p, _p, _p, _i, _p, _p, _cfgp]),
    "r2l_forward_poses_cfg": (_i, [_p, _i, _i, _i, _f, _p, _p, _p, _i, _p, _p, _cfgp]),
    "r2l_forward_emb": (_i, [_p, _p, _p, _i, _p, _p, _p, _l, _p]),
    "r2l_forward_emb_cfg": (_i, [_p, _p, _p, _i, _p, _p, _p, _l, _p, _p, _cfgp]),
    "r2l_num_tiles": (_l, [_l]),
    "r2l_padded_rows": (_l, [_l]),
    "r2l_stash_slot_floats": (_l, [_l]),
    "r2l_dw_slab_floats": (_l, []),
    "r2l_backward": (_i, [_p] * 12 + [_i, _f] + [_p] * 6 + [_l, _p]),
    "r2l_backward_part": (_i, [_p] * 12 + [_i, _f] + [_p] * 6 + [_l, _p, _i, _i, _i]),
    "r2l_backward_part_cfg": (_i, [_p] * 12 + [_i, _f] + [_p] * 6 + [_l, _p, _i, _i, _i, _cfgp]),
    "r2l_allreduce_unique_id": (_i, [_p]),
    "r2l_allreduce_init": (_i, [_p, _i, _i, _p]),
    "r2l_grad_allreduce": (_i, [_p, _p, _l, _p]),
    "r2l_allreduce_destroy": (_i, [_p]),
    "r2l_adam_step": (_i, [_p, _p, _p, _p, _l, _f, _f, _f, _f, _i, _f, _p]),
    "r2l_adam_step_guarded": (_i, [_p, _p, _p, _p, _l, _f, _f, _f, _f, _i, _f, _p, _p]),
    "r2l_adam_step_packed": (_i, [_p, _p, _p, _p, _i, _f, _f, _f, _f, _i, _f, _p, _p, _p, _p]),
    "r2l_chain_segments_ok_cfg": (_i, [_l, _i, _cfgp]),
    "r2l_backward_status_word": (_p, [_p, _i]),
    "r2l_backward_input": (_i, [_p, _p, _i, _p, _p, _p, _p, _p, _p, _p, _l, _p]),
    "r2l_forward_status_words": (_p, [_p, _i]),
    "r2l_backward_status_words": (_p, [_p, _i]),
    "r2l_teacher_status_words": (_p, [_p]),
    "r2l_loss_finish": (_i, [_p, _l, _f, _p, _p]),
    "r2l_teacher_param_count": (_l, []),
    "r2l_teacher_stream_floats": (_l, []),
    "r2l_pack_teacher": (_i, [_p, _p, _p]),
    "r2l_teacher_mlp": (_i, [_p, _p, _p, _p, _p, _p, _p, _l, _i, _p]),
    "r2l_teacher_mlp_cfg": (_i, [_p, _p, _p, _p, _p, _p, _p, _l, _i, _p, _cfgp]),
    "r2l_teacher_stash_floats": (_l, [_l]),
    "r2l_teacher_mlp_train": (_i, [_p, _p, _p, _p, _p, _p, _p, _p, _l, _i, _p]),
    "r2l_raw2outputs_backward": (_i, [_p, _p, _p, _p, _i, _p, _p, _p, _l, _i, _p]),
    "r2l_teacher_train_work_floats": (_l, [_l]),
    "r2l_teacher_backward": (_i, [_p] * 9 + [_l, _i, _p]),
    "r2l_raw2outputs_backward_scaled": (_i, [_p, _p, _p, _p, _i, _p, _p, _f, _p, _p, _p, _l, _i, _p]),
    "r2l_teacher_input_grad_work_floats": (_l, [_l]),
    "r2l_teacher_backward_input": (_i, [_p] * 8 + [_i] + [_p] * 5 + [_l, _i, _p]),
    "r2l_stratified_z": (_i, [_p, _p, _i, _p, _p, _p, _l, _i, _p]),
    "r2l_raw2outputs": (_i, [_p, _p, _p, _p, _i, _p, _p, _p, _p, _p, _l, _i, _p]),
    "r2l_sample_pdf_sort": (_i, [_p, _p, _p, _l, _p, _p, _p, _l, _i, _i, _p]),
    "r2l_draw_uniform": (_i, [_p, _l, ctypes.c_uint64, ctypes.c_uint64, _p]),
    "r2l_draw_normal": (_i, [_p, _l, ctypes.c_uint64, ctypes.c_uint64, _f, _p]),
    "r2l_ndc_rays": (_i, [_p, _p, _l, _i, _i, _f, _f, _p, _p, _p]),
    "r2l_frame_rays": (_i, [_p, _p, _f, _i, _i, _i, _p, _p, _p, _p, _p]),
    "r2l_teacher_frames_work_floats": (_l, [_descp]),
    "r2l_teacher_frames_cfg": (_i, [_p, _p, _i, _descp] + [_p] * 14 + [_cfgp]),
    "r2l_occ_bits_words": (_l, [_i]),
    "r2l_occ_grid_init": (_i, [_occp, _p, _i, _i, _p, _p]),
    "r2l_occ_build_work_floats": (_l, [_i, _i]),
    "r2l_occ_build": (_i, [_occp, _i, _i, _f, _p, _p, _cfgp, _p, _p, _p]),
    "r2l_occ_compact_work_bytes": (_l, [_l]),
    "r2l_occ_compact": (_i, [_occp] + [_p] * 4 + [_l, _i] + [_p] * 8),
    "r2l_occ_scatter": (_i, [_p, _p, _l, _p, _l, _i, _p]),
    "r2l_occ_index_work_bytes": (_l, [_l]),
    "r2l_occ_index": (_i, [_occp] + [_p] * 3 + [_l, _i] + [_p] * 4),
    "r2l_occ_live_add": (_i, [_p, _l, _p, _p]),
    "r2l_occ_rays_work_bytes": (_l, [_l]),
    "r2l_occ_rays": (_i, [_occp, _p, _p, _l, _f, _f, _i, _p, _p, _p, _p, _p]),
    "r2l_rays_gather": (_i, [_p, _p, _l, _p, _l, _p, _p, _p]),
    "r2l_rgb_scatter_bg": (_i, [_p, _p, _l, _p, _f, _p, _l, _p]),
    "r2l_store_append_live": (_i, [_p, _l, _p, _l, _p, _l, _l, _l, ctypes.c_uint64, _i, _p, _p]),
    "r2l_teacher_mlp_live_cfg": (_i, [_p] * 9 + [_l, _i, _p, _cfgp]),
    "r2l_teacher_frames_occ_work_floats": (_l, [_descp]),
    "r2l_teacher_frames_occ_cfg": (_i, [_p, _p, _i, _descp] + [_p] * 12 + [_occp, _occp, _p, _p, _p, _cfgp]),
    "r2l_occ_index_seg_work_bytes": (_l, [_l]),
    "r2l_occ_index_seg": (_i, [_occp] + [_p] * 3 + [_l, _i, _i, _i, _p, _f] + [_p] * 4),
    "r2l_ert_advance": (_i, [_p, _p, _p, _l, _i, _i, _i, _p, _p]),
    "r2l_teacher_mlp_live_into_cfg": (_i, [_p] * 6 + [_l] + [_p] * 3 + [_l, _i, _p, _cfgp]),
    "r2l_teacher_frames_ert_work_floats": (_l, [_descp, _ertp]),
    "r2l_teacher_frames_ert_cfg": (_i, [_p, _p, _i, _descp] + [_p] * 12 + [_occp, _occp, _p, _ertp, _p, _p, _cfgp]),
    "r2l_ssim_partial_count": (_l, [_i, _i, _i]),
    "r2l_ssim": (_i, [_p, _p, _i, _i, _i, _p, _p, _p, _p]),
    "r2l_flip_partial_count": (_l, [_i, _i, _i]),
    "r2l_flip": (_i, [_p, _p, _i, _i, _i, _f, _p, _p, _p, _p, _p]),
    "r2l_lpips_param_floats": (_l, []),
    "r2l_lpips_pack_floats": (_l, []),
    "r2l_lpips_pack": (_i, [_p, _p, _p]),
    "r2l_lpips_work_floats": (_l, [_i, _i, _i]),
    "r2l_lpips_map_floats": (_l, [_i, _i]),
    "r2l_lpips": (_i, [_p, _p, _i, _i, _i, _p, _p, _p, _p, _p, _p, _p]),
    "r2l_lpips_vgg_param_floats": (_l, []),
    "r2l_lpips_vgg_pack_floats": (_l, []),
    "r2l_lpips_vgg_pack": (_i, [_p, _p, _p]),
    "r2l_lpips_vgg_work_floats": (_l, [_i, _i, _i]),
    "r2l_lpips_vgg_map_floats": (_l, [_i, _i]),
    "r2l_lpips_vgg": (_i, [_p, _p, _i, _i, _i, _p, _p, _p, _p, _p, _p, _p]),
    "r2l_pool_pick": (_i, [_p, _l, _l, ctypes.c_uint64, _p]),
    "r2l_pool_augment": (_i, [_p, _p, _p, _l, _l, _l, _p, _p, _l, _l, _p, _p, _p, _p]),
    "r2l_pool_store": (_i, [_p, _p, _p, _l, _l, _l, _p, _p, _p, _l, _l, _p]),
    "r2l_pool_select_work_bytes": (_l, [_l]),
    "r2l_pool_select": (_i, [_p, _p, _l, _l, _l, _l, _p, _p, _p, _p]),
    "r2l_store_append": (_i, [_p, _l, _p, _l, _l, _l, ctypes.c_uint64, _i, _p, _p]),
    "r2l_store_batch": (_i, [_p, _l, _l, _l, _l, ctypes.c_uint64, _p, _p, _p]),
    "r2l_store_append_images": (_i, [_p, _p, _p, _f, _i, _i, _i, _p, _l, _l, _l, ctypes.c_uint64, _i, _p, _p]),
    "r2l_cstore_append": (_i, [_cstorep, _p, _l, _p, _p, _f, _i, _l, _l, ctypes.c_uint64, _i, _p, _p]),
    "r2l_cstore_batch": (_i, [_cstorep, _l, _l, _l, ctypes.c_uint64, _p, _p, _p]),
    "r2l_words_digest": (_i, [_p, _l, _l, ctypes.c_uint64, _p, _p]),
    "r2l_train_batch": (_i, [_p, _l, _l, _l, _l, ctypes.c_uint64, _p, _l, _l, ctypes.c_uint64, _p, _p, _p, _p, _p, _p]),
    "r2l_student_step_work_floats": (_l, [_sstepp]),
    "r2l_student_train_step": (_i, [_sstepp] + [_p] * 13),
    "r2l_pixel_batch": (_i, [_p, _p, _i, _i, _i, _f, _i, _l, _l, ctypes.c_uint64, _p, _p, _p, _p, _p, _p]),
    "r2l_image_batch": (_i, [_p, _p, _i, _i, _i, _f, _i, _i, _i, _i, _i, _i, ctypes.c_uint64, _l, _p, _p, _p, _p, _p, _p]),
    "r2l_image_draw": (_i, [ctypes.c_uint64, _l, _i, _p, _p]),
    "r2l_pose_key": (_i, [ctypes.c_uint64, _l, _l, _p]),
    "r2l_pose_batch": (_i, [_p, _p, _i, _i, _i, _f, ctypes.c_uint64, _l, _l, _p, _p, _p, _p, _p]),
    "r2l_pose_grad_work_floats": (_l, [_l, _l]),
    "r2l_pose_grad": (_i, [_p, _p, _p, _p, _p, _l, _l, _p, _p, _p, _p]),
    "r2l_pose_update": (_i, [_p, _p, _p, _p, _i, _f, _f, _f, _f, _f, _l, _p]),
    "r2l_pose_refine_work_floats": (_l, [_posep]),
    "r2l_pose_refine_step": (_i, [_posep] + [_p] * 11),
    "r2l_teacher_step_work_floats": (_l, [_stepp]),
    "r2l_teacher_train_step": (_i, [_stepp] + [_p] * 15),
    "r2l_teacher_mlp_train_live": (_i, [_p] * 10 + [_l, _i, _p]),
    "r2l_teacher_train_live_work_floats": (_l, [_l]),
    "r2l_teacher_backward_live": (_i, [_p] * 11 + [_l, _i, _p]),
    "r2l_teacher_step_occ_work_floats": (_l, [_stepp]),
    "r2l_teacher_train_step_occ": (_i, [_stepp] + [_p] * 13 + [_occp, _occp, _p, _p, _p]),
    "r2l_png_writer_open": (_i, [_i, _i, _p]),
    "r2l_png_writer_submit": (_i, [_p, ctypes.c_char_p, _p, _i, _i, _i, _p, _p]),
    "r2l_png_writer_wait": (_i, [_p, _l]),
    "r2l_png_writer_close": (_i, [_p]),
    "r2l_npy_shape": (_i, [ctypes.c_char_p, _p, _p]),
    "r2l_reader_open": (_i, [_p, _l, _i, _i, ctypes.c_uint64, _p, _i, _p]),
    "r2l_reader_info": (_i, [_p, _p, _p, _p]),
    "r2l_reader_next": (_i, [_p, _p]),
    "r2l_reader_release": (_i, [_p, _i]),
    "r2l_reader_close": (_i, [_p]),
}

# range control of the fp16 kernels (include/r2l_hip.h "range control"; csrc/r2l_common.h F2S_* / B2S_*): the word that marks a
# status area as initialised, and the decoding of the forward / teacher area's 16 words
RANGE_MAGIC = 0x52324c34


def decode_range_words(w):
    """w: the 16 status words as an int32 CPU tensor -> {'amax', 'scale', 'headroom', 'trips', 'rescales', 'flag'}."""
    import torch
    f = w.view(torch.float32)
    scale = float(f[2]) if int(w[4]) == RANGE_MAGIC else 1.0
    live = float(f[1]) * scale
    amax = live if live > 0 else float(f[6])
    return {"amax": amax, "scale": scale, "headroom": (32768.0 * scale / amax) if amax > 0 else float("inf"),
            "trips": int(w[5]), "rescales": int(w[7]), "flag": int(w[0])}


# stage bits of r2l_backward_part (include/r2l_hip.h)
BWD_CHAIN, BWD_BODY, BWD_HEAD, BWD_TAIL, BWD_ALL, BWD_NOFALLBACK = 1, 2, 4, 8, 15, 16

_lib = None


def load():
    """Load the library once and bind every export; raises RuntimeError if anything is missing."""
    global _lib
    if _lib is not None:
        return _lib
    # PyTorch bundles its own libamdhip64 (same soname as /opt/rocm's).  It must be the one the process loads FIRST:
    # if libr2l_hip.so pulled in the system runtime before torch was imported, torch would bind to that copy and fail
    # with "no ROCm-capable device is detected".  One HIP runtime per process: torch's.
    import torch  # noqa: F401
    if not os.path.exists(LIB_PATH):
        raise RuntimeError(
            "libr2l_hip.so not found at %s — build it with `python -m r2l_amd.build` "
            "(or __graft_entry__.build()); there is no non-HIP fallback for the R2L hot path." % LIB_PATH)
    lib = ctypes.CDLL(LIB_PATH)
    for name, (res, args) in SIGNATURES.items():
        try:
            fn = getattr(lib, name)
        except AttributeError as e:
            raise RuntimeError("libr2l_hip.so lacks export %s" % name) from e
        fn.restype = res
        fn.argtypes = args
    _lib = lib
    return lib


def ptr(t):
    """The address of a tensor's data as a c_void_p; None (a null pointer argument) for None."""
    return ctypes.c_void_p(t.data_ptr()) if t is not None else None


def stream(device=None):
    """The current stream of `device` (None: of the current device) as a c_void_p."""
    import torch
    return ctypes.c_void_p(torch.cuda.current_stream(device).cuda_stream)


def check(code, what):
    if code != 0:
        msg = load().r2l_last_error()
        raise RuntimeError("%s failed: hip error %d: %s" % (what, code, msg.decode() if msg else "?"))
