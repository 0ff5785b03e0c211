"""ctypes binding of libsda_hip.so (the C ABI declared in include/sda_hip.h).

The product path has NO fallback: if the library is missing or a symbol does not resolve,
loading raises -- nothing in sda_amd computes on the CPU or through the oracle.
"""
import ctypes
import os
from ctypes import POINTER, Structure, c_double, c_float, c_int, c_int32, c_int64, c_uint32, c_uint64, c_void_p

import torch  # noqa: F401  -- must be imported first: the library binds to the HIP runtime torch loaded

HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get('SDA_HIP_LIB') or os.path.join(HERE, 'lib', 'libsda_hip.so')     # (SDA_HIP_LIB: a tooling build, tools/ only)

ACT_IDS = {None: 0, 'none': 0, 'SiLU': 1, 'ReLU': 2, 'ELU': 3, 'GELU': 4, 'SELU': 5}

c_fp = c_void_p  # device pointers travel as integers


class ConvDesc(Structure):
    """Mirror of `struct sda_conv_desc` (include/sda_hip.h) -- field order and types must match."""
    _fields_ = [
        ('x', c_fp),
        ('x_sn_outer', c_int64), ('x_sn_inner', c_int64),
        ('n_inner', c_int32),
        ('x_n_off', c_int32),
        ('x_sc', c_int64), ('x_sy', c_int64), ('x_sx', c_int64),
        ('cx', c_int32),
        ('ctx', c_fp),
        ('ctx_sn', c_int64),
        ('cctx', c_int32),
        ('n', c_int32),
        ('hs', c_int32), ('ws', c_int32),
        ('up_h', c_int32), ('up_w', c_int32),
        ('zins_h', c_int32), ('zins_w', c_int32),
        ('mod', c_fp),
        ('mod_sn', c_int64),
        ('ln_mean', c_fp),
        ('ln_rstd', c_fp),
        ('act_in', c_int32),
        ('kh', c_int32), ('kw', c_int32), ('stride_h', c_int32), ('stride_w', c_int32), ('circular', c_int32),
        ('w', c_fp),
        ('cin_pad', c_int32), ('cout_pad', c_int32),
        ('bias', c_fp),
        ('out', c_fp),
        ('cout', c_int32), ('ho', c_int32), ('wo', c_int32),
        ('dact_z', c_fp),
        ('act_d', c_int32),
        ('res', c_fp),
        ('mt', c_int32),
        ('explicit_pad', c_int32), ('pad_h', c_int32), ('pad_w', c_int32),
        ('out_sn', c_int64), ('out_sc', c_int64), ('out_sy', c_int64), ('out_sx', c_int64),
        ('w_wino4', c_fp),
        ('pool_h', ctypes.c_int32), ('pool_w', ctypes.c_int32),
        ('w_wino4_zp', c_fp),
        ('w_h2', ctypes.c_void_p), ('w_h2_scale', ctypes.c_float), ('x_amax_static', ctypes.c_float),
        ('x_amax', c_fp), ('out_amax', c_fp),
    ]


class Conv3dDesc(Structure):
    """Mirror of `struct sda_conv3d_desc` (include/sda_hip.h)."""
    _fields_ = [
        ('x', c_fp), ('w', c_fp), ('bias', c_fp), ('z', c_fp), ('res', c_fp), ('out', c_fp),
        ('n', c_int32), ('cin', c_int32), ('cout', c_int32),
        ('in_size', c_int32 * 3), ('out_size', c_int32 * 3),
        ('k', c_int32 * 3), ('pad', c_int32 * 3), ('stride', c_int32 * 3), ('up', c_int32 * 3), ('dil', c_int32 * 3),
        ('circular', c_int32), ('act', c_int32), ('act_in', c_int32),
    ]


# name -> (restype, argtypes); exactly the symbols include/sda_hip.h declares
class Block1dDesc(Structure):
    """Mirror of `struct sda_block1d_desc` (include/sda_hip.h)."""
    _fields_ = [
        ('n', c_int32), ('c', c_int32), ('len', c_int32),
        ('circular', c_int32), ('act', c_int32), ('unbiased', c_int32),
        ('eps', c_float),
        ('k_pad', c_int32), ('m_pad', c_int32),
        ('a', c_fp),
        ('mod', c_fp),
        ('mod_sn', c_int64),
        ('w1', c_fp), ('b1', c_fp),
        ('w2', c_fp), ('b2', c_fp),
        ('z', c_fp),
        ('mean', c_fp), ('rstd', c_fp),
        ('y', c_fp),
        ('g', c_fp),
        ('gx', c_fp),
    ]


NET1D_MAXB = 8


class Net1dDesc(Structure):
    """Mirror of `struct sda_net1d_desc` (include/sda_hip.h)."""
    _fields_ = [
        ('n', c_int32), ('len', c_int32),
        ('cin', c_int32), ('c', c_int32), ('cout', c_int32),
        ('nblocks', c_int32),
        ('circular', c_int32), ('act', c_int32), ('unbiased', c_int32),
        ('eps', c_float),
        ('x', c_fp), ('x_sn', c_int64), ('x_sc', c_int64), ('x_sx', c_int64),
        ('out', c_fp), ('out_sn', c_int64), ('out_sc', c_int64), ('out_sx', c_int64),
        ('w', c_fp),
        ('bias', c_fp),
        ('mod', c_fp * NET1D_MAXB),
        ('mod_sn', c_int64),
        ('a_save', c_fp), ('z_save', c_fp), ('save_stride', c_int64),
        ('mean_save', c_fp), ('rstd_save', c_fp), ('stat_stride', c_int64),
    ]


class Net1dTrainDesc(Structure):
    """Mirror of `struct sda_net1d_train_desc` (include/sda_hip.h)."""
    _fields_ = [('net', Net1dDesc), ('tail_in', c_fp), ('g_save', c_fp), ('g_stride', c_int64), ('mod_part', c_fp), ('mod_tiles', c_int32)]


NET1D_MAXV = 2 + 2 * NET1D_MAXB


class Net1dWgradDesc(Structure):
    """Mirror of `struct sda_net1d_wgrad_desc` (include/sda_hip.h)."""
    _fields_ = [
        ('net', Net1dDesc),
        ('tail_in', c_fp),
        ('g_save', c_fp), ('g_stride', c_int64),
        ('gout', c_fp), ('gout_sn', c_int64), ('gout_sc', c_int64), ('gout_sx', c_int64),
        ('mod_part', c_fp), ('mod_tiles', c_int32),
        ('dw', c_fp * NET1D_MAXV),
        ('db', c_fp * NET1D_MAXV),
        ('dmod', c_fp * NET1D_MAXB), ('dmod_sn', c_int64),
        ('work', c_fp),
        ('slabs', c_int32),
    ]


class Net1dPackDesc(Structure):
    """Mirror of `struct sda_net1d_pack_desc` (include/sda_hip.h)."""
    _fields_ = [
        ('nblocks', c_int32), ('cin', c_int32), ('c', c_int32), ('cout', c_int32), ('cin_keep', c_int32),
        ('w', c_fp * NET1D_MAXV),
        ('b', c_fp * NET1D_MAXV),
        ('wf', c_fp), ('wb', c_fp), ('bias', c_fp),
    ]


MLP_MAXG = 32


class MlpDesc(Structure):
    """Mirror of `struct sda_mlp_desc` (include/sda_hip.h)."""
    _fields_ = [
        ('rows', c_int32), ('ngemm', c_int32),
        ('act', c_int32), ('unbiased', c_int32),
        ('eps', c_float),
        ('kind', c_int32 * MLP_MAXG),
        ('in_f', c_int32 * MLP_MAXG), ('out_f', c_int32 * MLP_MAXG),
        ('w_off', c_int32 * MLP_MAXG), ('b_off', c_int32 * MLP_MAXG),
        ('w', c_fp), ('bias', c_fp),
        ('x', c_fp), ('x_ld', c_int64),
        ('out', c_fp), ('out_ld', c_int64),
        ('a_save', c_fp), ('z_save', c_fp), ('save_stride', c_int64), ('save_ld', c_int32),
        ('mean_save', c_fp), ('rstd_save', c_fp), ('stat_stride', c_int64),
    ]


class MlpTrainDesc(Structure):
    """Mirror of `struct sda_mlp_train_desc` (include/sda_hip.h)."""
    _fields_ = [('mlp', MlpDesc), ('g_save', c_fp), ('g_stride', c_int64), ('g_ld', c_int32)]


class MlpWgradDesc(Structure):
    """Mirror of `struct sda_mlp_wgrad_desc` (include/sda_hip.h)."""
    _fields_ = [
        ('rows', c_int32), ('ngemm', c_int32),
        ('act', c_int32),
        ('kind', c_int32 * MLP_MAXG),
        ('in_f', c_int32 * MLP_MAXG), ('out_f', c_int32 * MLP_MAXG),
        ('src', c_fp * MLP_MAXG), ('src_ld', c_int64 * MLP_MAXG),
        ('mean', c_fp * MLP_MAXG), ('rstd', c_fp * MLP_MAXG),
        ('g', c_fp * MLP_MAXG), ('g_ld', c_int64),
        ('dw', c_fp * MLP_MAXG), ('db', c_fp * MLP_MAXG),
        ('work', c_fp),
        ('slabs', c_int32), ('accumulate', c_int32),
    ]


ADAMW_MAXT = 32


class AdamWDesc(Structure):
    """Mirror of `struct sda_adamw_desc` (include/sda_hip.h)."""
    _fields_ = [
        ('ntensor', c_int32),
        ('decay', c_float), ('one_m_beta1', c_float), ('beta2', c_float), ('one_m_beta2', c_float),
        ('step_size', c_float), ('rsqrt_bc2', c_float), ('eps', c_float),
        ('p', c_fp * ADAMW_MAXT), ('g', c_fp * ADAMW_MAXT), ('m', c_fp * ADAMW_MAXT), ('v', c_fp * ADAMW_MAXT),
        ('fwd', c_fp * ADAMW_MAXT), ('bwd', c_fp * ADAMW_MAXT),
        ('numel', c_int64 * ADAMW_MAXT),
        ('pack_kind', c_int32 * ADAMW_MAXT),
        ('out_f', c_int32 * ADAMW_MAXT), ('in_f', c_int32 * ADAMW_MAXT),
        ('blk0', c_int32 * (ADAMW_MAXT + 1)),
    ]


class MlpWin(Structure):
    """Mirror of `struct sda_mlp_win` (include/sda_hip.h)."""
    _fields_ = [
        ('nw', c_int32), ('len', c_int32), ('c', c_int32), ('emb_n', c_int32),
        ('x', c_fp), ('emb', c_fp),
        ('cx0', c_float), ('cx1', c_float), ('cn', c_float),
        ('coef', c_fp),
        ('y', c_fp), ('y_sn', c_int64),
        ('p_start', c_int32), ('p_step', c_int32), ('p_stop', c_int32),
        ('c_start', c_int32), ('c_step', c_int32), ('c_stop', c_int32),
        ('std', c_float), ('gamma', c_float),
        ('eps', c_fp), ('ghat', c_fp),
        ('gwin', c_fp),
    ]


class Net1dFuse(Structure):
    """Mirror of `struct sda_net1d_fuse` (include/sda_hip.h)."""
    _fields_ = [
        ('cx0', c_float), ('cx1', c_float), ('cn', c_float),
        ('coef', c_fp),
        ('y', c_fp), ('y_sn', c_int64),
        ('p_start', c_int32), ('p_step', c_int32), ('p_stop', c_int32),
        ('c_start', c_int32), ('c_step', c_int32), ('c_stop', c_int32),
        ('std', c_float), ('gamma', c_float),
        ('ghat', c_fp),
        ('eps', c_fp),
        ('mode', c_int32),
        ('xs', c_fp),
        ('step_coef', c_fp),
        ('partial', c_fp), ('partial_stride', c_int32),
    ]


class WgradDesc(Structure):
    """include/sda_hip.h sda_wgrad_desc"""
    _fields_ = [
        ('conv', ConvDesc),
        ('g', c_fp), ('dw', c_fp), ('db', c_fp), ('work', c_fp),
        ('slabs', c_int32), ('accumulate', c_int32),
    ]


CHAIN_KINDS = {'lorenz63': 0, 'lotka_volterra': 1, 'lorenz96': 2}
CHAIN_MAXOBS = 64


class ChainModel(Structure):
    """Mirror of `struct sda_chain_model` (include/sda_hip.h)."""
    _fields_ = [('kind', c_int32), ('d', c_int32), ('steps', c_int32), ('h', c_float), ('p', c_float * 4), ('noise_std', c_float)]


class ChainObs(Structure):
    """Mirror of `struct sda_chain_obs` (include/sda_hip.h)."""
    _fields_ = [('k', c_int32), ('idx', c_int32 * CHAIN_MAXOBS), ('shift', c_float * CHAIN_MAXOBS), ('scale', c_float * CHAIN_MAXOBS),
                ('sigma', c_float), ('y', c_fp)]


class ChainAdv(Structure):
    """Mirror of `struct sda_chain_adv` (include/sda_hip.h)."""
    _fields_ = [
        ('model', ChainModel),
        ('x_in', c_fp), ('in_sp', c_int64), ('anc', c_fp),
        ('out', c_fp), ('out_st', c_int64), ('out_sp', c_int64),
        ('every', c_int32),
        ('m', c_int32), ('transitions', c_int32),
        ('seed', c_uint64), ('row0', c_int64), ('draw0', c_int64),
        ('obs', POINTER(ChainObs)),
        ('logw', c_fp), ('pmax', c_fp),
    ]


class ChainVjp(Structure):
    """Mirror of `struct sda_chain_vjp` (include/sda_hip.h)."""
    _fields_ = [
        ('model', ChainModel),
        ('x_in', c_fp), ('in_sp', c_int64), ('anc', c_fp),
        ('states', c_fp), ('st_st', c_int64), ('st_sp', c_int64),
        ('g', c_fp), ('g_st', c_int64), ('g_sp', c_int64),
        ('every', c_int32),
        ('m', c_int32), ('transitions', c_int32),
        ('gx', c_fp), ('gx_sp', c_int64),
    ]


class KflowModel(Structure):
    """Mirror of `struct sda_kflow_model` (include/sda_hip.h)."""
    _fields_ = [('n', c_int32), ('steps', c_int32), ('delta', c_float), ('nu', c_float), ('hm', c_fp), ('inv', c_fp), ('forcing', c_fp)]


LGSS_MAXD = 8


class LgssModel(Structure):
    """Mirror of `struct sda_lgss_model` (include/sda_hip.h)."""
    _fields_ = [('d', c_int32), ('A', c_float * LGSS_MAXD * LGSS_MAXD), ('b', c_float * LGSS_MAXD), ('Lq', c_float * LGSS_MAXD * LGSS_MAXD)]


class LgssModel64(Structure):
    """Mirror of `struct sda_lgss_model64` (include/sda_hip.h)."""
    _fields_ = [('d', c_int32), ('k', c_int32),
                ('A', c_double * LGSS_MAXD * LGSS_MAXD), ('b', c_double * LGSS_MAXD), ('Q', c_double * LGSS_MAXD * LGSS_MAXD),
                ('m0', c_double * LGSS_MAXD), ('P0', c_double * LGSS_MAXD * LGSS_MAXD),
                ('H', c_double * LGSS_MAXD * LGSS_MAXD), ('c', c_double * LGSS_MAXD),
                ('sigma', c_double)]


SIGNATURES = {
    'sda_abi_version': (c_int, []),
    'sda_conv_igemm': (c_int, [POINTER(ConvDesc), c_void_p]),
    'sda_gauss_cotangent': (c_int, [c_void_p, c_int64, c_void_p, c_int64, c_float, c_float, c_float, c_float, c_void_p, c_void_p, c_void_p]),
    'sda_block1d_fwd': (c_int, [POINTER(Block1dDesc), c_void_p]),
    'sda_block1d_bwd': (c_int, [POINTER(Block1dDesc), c_void_p]),
    'sda_block1d_tile': (c_int, [POINTER(Block1dDesc)]),
    'sda_net1d_fwd': (c_int, [POINTER(Net1dDesc), c_void_p]),
    'sda_net1d_bwd': (c_int, [POINTER(Net1dDesc), c_void_p]),
    'sda_net1d_fwd_fused': (c_int, [POINTER(Net1dDesc), POINTER(Net1dFuse), c_void_p]),
    'sda_net1d_bwd_fused': (c_int, [POINTER(Net1dDesc), POINTER(Net1dFuse), c_void_p]),
    'sda_net1d_tiles': (c_int, [POINTER(Net1dDesc)]),
    'sda_net1d_fwd_train': (c_int, [POINTER(Net1dTrainDesc), c_void_p]),
    'sda_net1d_bwd_train': (c_int, [POINTER(Net1dTrainDesc), c_void_p]),
    'sda_net1d_wgrad': (c_int, [POINTER(Net1dWgradDesc), c_void_p]),
    'sda_net1d_wgrad_slabs': (c_int, [POINTER(Net1dWgradDesc)]),
    'sda_net1d_wgrad_work_floats': (c_int64, [POINTER(Net1dWgradDesc)]),
    'sda_net1d_pack': (c_int, [POINTER(Net1dPackDesc), c_void_p]),
    'sda_step1d_prologue': (c_int, [c_fp, c_int, c_fp, c_fp, c_int, c_int, c_float, c_float, c_int, c_fp, c_int, c_fp, c_fp, c_int,
                                    c_fp, c_fp, c_int, c_fp, c_fp, c_int, c_fp, c_fp, c_fp, c_void_p]),
    'sda_step1d_prologue_path': (c_int, [c_int, c_int, c_int, c_int, c_fp, c_fp, c_fp]),
    'sda_pc_correct_keyed': (c_int, [c_fp, c_fp, c_int, c_int64, c_fp, c_int, c_float, c_float, c_fp, c_uint64, c_int64, c_fp, c_int64,
                                     c_int64, c_void_p]),
    'sda_conv_parity4': (c_int, [POINTER(ConvDesc), c_void_p]),
    'sda_conv_igemm_path': (c_int, [POINTER(ConvDesc)]),
    'sda_small1d_tile': (c_int, [POINTER(ConvDesc)]),
    'sda_conv_wgrad': (c_int, [POINTER(WgradDesc), c_void_p]),
    'sda_conv_wgrad_slabs': (c_int, [POINTER(WgradDesc)]),
    'sda_conv_wgrad_work_floats': (c_int64, [POINTER(WgradDesc)]),
    'sda_conv_wgrad3_serves': (c_int, [POINTER(WgradDesc)]),
    'sda_conv_wgrad3_work_floats': (c_int64, [POINTER(WgradDesc)]),
    'sda_conv_wgrad3': (c_int, [POINTER(WgradDesc), c_void_p]),
    'sda_conv_wgrad3x_serves': (c_int, [POINTER(WgradDesc)]),
    'sda_conv_wgrad3x_work_floats': (c_int64, [POINTER(WgradDesc)]),
    'sda_conv_wgrad3x': (c_int, [POINTER(WgradDesc), c_void_p]),
    'sda_plane_sum': (c_int, [c_fp, c_fp, c_int, c_int, c_int64, c_fp, c_int64, c_int, c_int, c_void_p]),
    'sda_conv_igemm_lds_bytes': (c_int64, [POINTER(ConvDesc)]),
    'sda_pack_conv_weight': (c_int, [c_fp, c_int, c_int, c_int, c_int, c_int, c_int, c_fp, c_int, c_int, c_void_p]),
    'sda_pack_conv_weight_wino4': (c_int, [c_fp, c_int, c_int, c_int, c_int, c_fp, c_int, c_int, c_void_p]),
    'sda_pack_conv_weight_wino4_zp': (c_int, [c_fp, c_int, c_int, c_fp, c_void_p]),
    'sda_wino4_zp_floats': (c_int64, [c_int, c_int]),
    'sda_ln_stats': (c_int, [c_fp, c_int, c_int, c_int, c_fp, c_int64, c_float, c_int, c_fp, c_fp, c_void_p]),
    'sda_ln_apply': (c_int, [c_fp, c_int, c_int, c_int, c_fp, c_int64, c_fp, c_fp, c_fp, c_void_p]),
    'sda_ln_bwd': (c_int, [c_fp, c_fp, c_int, c_int, c_int, c_int, c_fp, c_int64, c_fp, c_fp, c_int, c_int, c_int, c_fp, c_fp,
                           c_void_p]),
    'sda_ln_bwd_amax': (c_int, [c_fp, c_fp, c_int, c_int, c_int, c_int, c_fp, c_int64, c_fp, c_fp, c_int, c_int, c_int, c_fp, c_fp,
                           c_fp, c_void_p]),
    'sda_time_embed': (c_int, [c_fp, c_int, c_fp, c_int, c_fp, c_fp, c_int, c_fp, c_fp, c_int, c_fp, c_void_p]),
    'sda_linear_small': (c_int, [c_fp, c_int, c_int, c_fp, c_fp, c_int, c_fp, c_void_p]),
    'sda_linear': (c_int, [c_fp, c_int, c_int, c_fp, c_fp, c_int, c_int, c_int, c_int, c_fp, c_int, c_fp, c_fp, c_void_p]),
    'sda_mlp_fwd': (c_int, [POINTER(MlpDesc), c_void_p]),
    'sda_mlp_bwd': (c_int, [POINTER(MlpDesc), c_void_p]),
    'sda_mlp_slab_floats': (c_int, [c_int, c_int]),
    'sda_mlp_bwd_train': (c_int, [POINTER(MlpTrainDesc), c_void_p]),
    'sda_mlp_wgrad': (c_int, [POINTER(MlpWgradDesc), c_void_p]),
    'sda_mlp_wgrad_slabs': (c_int, [POINTER(MlpWgradDesc)]),
    'sda_mlp_wgrad_work_floats': (c_int64, [POINTER(MlpWgradDesc)]),
    'sda_adamw_step': (c_int, [POINTER(AdamWDesc), c_void_p]),
    'sda_adamw_step_dev': (c_int, [POINTER(AdamWDesc), c_fp, c_fp, c_void_p]),
    'sda_loss_perturb': (c_int, [c_fp, c_int, c_int64, c_uint64, c_int64, c_int64, c_fp, c_int, c_float, c_float, c_int, c_fp, c_fp, c_fp, c_void_p]),
    'sda_loss_mse_plan': (c_int64, [c_int64, POINTER(c_int), POINTER(c_int)]),
    'sda_loss_mse': (c_int, [c_fp, c_fp, c_int64, c_fp, c_fp, c_fp, c_void_p]),
    'sda_window_batch': (c_int, [c_fp, c_int64, c_int64, c_int64, c_int64, c_int64, c_int64, c_uint64, c_int64, c_fp, c_fp, c_void_p]),
    'sda_window_batch_plan': (c_int, [c_int64, c_int64, c_int64, c_int64, c_uint64, c_int64, c_int64, POINTER(c_int64), POINTER(c_int64)]),
    'sda_mlp_fwd_win': (c_int, [POINTER(MlpDesc), POINTER(MlpWin), c_void_p]),
    'sda_mlp_bwd_win': (c_int, [POINTER(MlpDesc), POINTER(MlpWin), c_void_p]),
    'sda_mc_finish': (c_int, [c_fp, c_fp, c_fp, c_int, c_int, c_int, c_int, c_float, c_float, c_fp, c_int, c_fp, c_fp, c_fp, c_fp, c_void_p]),
    'sda_row_ln': (c_int, [c_fp, c_int, c_int, c_float, c_int, c_fp, c_fp, c_fp, c_void_p]),
    'sda_row_ln_bwd': (c_int, [c_fp, c_fp, c_int, c_int, c_fp, c_fp, c_int, c_fp, c_fp, c_void_p]),
    'sda_obs_subsample': (c_int, [c_fp, POINTER(c_int), POINTER(c_int), POINTER(c_int), POINTER(c_int), c_fp, c_void_p]),
    'sda_obs_subsample_adjoint': (c_int, [c_fp, POINTER(c_int), POINTER(c_int), POINTER(c_int), POINTER(c_int), c_fp, c_void_p]),
    'sda_obs_pointwise': (c_int, [c_fp, c_int64, c_int, c_fp, c_void_p]),
    'sda_obs_pointwise_vjp': (c_int, [c_fp, c_fp, c_int64, c_int, c_fp, c_void_p]),
    'sda_obs_mask': (c_int, [c_fp, c_int64, c_fp, c_int64, c_fp, c_void_p]),
    'sda_obs_timediff': (c_int, [c_fp, c_int64, c_int, c_int64, c_int, c_int, c_fp, c_void_p]),
    'sda_obs_timediff_adjoint': (c_int, [c_fp, c_int64, c_int, c_int64, c_int, c_int, c_fp, c_void_p]),
    'sda_obs_subsample_guidance': (c_int, [c_fp, c_fp, c_fp, c_int64, POINTER(c_int), POINTER(c_int), POINTER(c_int), POINTER(c_int),
                                           c_float, c_float, c_float, c_float, c_fp, c_fp, c_void_p]),
    'sda_obs_coarsen': (c_int, [c_fp, c_int64, c_int, c_int, c_int, c_fp, c_void_p]),
    'sda_obs_coarsen_adjoint': (c_int, [c_fp, c_int64, c_int, c_int, c_int, c_fp, c_void_p]),
    'sda_obs_vorticity': (c_int, [c_fp, c_int64, c_int, c_int, c_fp, c_void_p]),
    'sda_obs_vorticity_adjoint': (c_int, [c_fp, c_int64, c_int, c_int, c_fp, c_void_p]),
    'sda_fold': (c_int, [c_fp, c_int, c_int, c_int, c_int, c_int, c_fp, c_void_p]),
    'sda_fold_adjoint': (c_int, [c_fp, c_int, c_int, c_int, c_int, c_int, c_fp, c_void_p]),
    'sda_unfold_adjoint': (c_int, [c_fp, c_int, c_int, c_int, c_int, c_int, c_int64, c_fp, c_void_p]),
    'sda_vp_schedule': (c_int, [c_fp, c_int, c_float, c_float, c_int, c_fp, c_void_p]),
    'sda_pc_predict': (c_int, [c_fp, c_fp, c_int64, c_float, c_float, c_fp, c_void_p]),
    'sda_sumsq_partial': (c_int, [c_fp, c_int, c_int64, c_fp, c_int, c_void_p]),
    'sda_pc_correct': (c_int, [c_fp, c_fp, c_fp, c_int, c_int64, c_fp, c_int, c_float, c_float, c_fp, c_void_p]),
    'sda_randn_rows': (c_int, [c_fp, c_int, c_int64, c_uint64, c_int64, c_int64, c_fp, c_int64, c_int64, c_void_p]),
    'sda_clock_probe': (c_int, [c_void_p, c_int, c_void_p, c_int, c_void_p]),
    'sda_conv_h2': (c_int, [POINTER(ConvDesc), c_void_p]),
    'sda_conv_h2_supported': (c_int, [POINTER(ConvDesc)]),
    'sda_pack_conv_weight_h2': (c_int, [c_fp, c_int, c_int, c_int, c_float, c_void_p, c_void_p]),
    'sda_conv_h2_packed_bytes': (c_int64, [c_int, c_int, c_int]),
    'sda_pack_conv_weight_h2_up': (c_int, [c_fp, c_int, c_int, c_float, c_void_p, c_void_p]),
    'sda_conv_h2_up_packed_bytes': (c_int64, [c_int, c_int]),
    'sda_pack_conv_weight_h2_rows': (c_int, [c_fp, c_int, c_int, c_int, c_float, c_void_p, c_void_p]),
    'sda_conv_h2_rows_packed_bytes': (c_int64, [c_int, c_int, c_int]),
    'sda_conv_h2_scale': (c_float, [c_float]),
    'sda_absmax': (c_int, [c_fp, c_int64, c_fp, c_void_p]),
    'sda_philox_words': (c_int, [c_fp, c_int64, c_uint64, c_uint32, c_uint32, c_uint32, c_void_p]),
    'sda_denoise': (c_int, [c_fp, c_fp, c_int64, c_float, c_float, c_fp, c_fp, c_void_p]),
    'sda_guided_combine': (c_int, [c_fp, c_fp, c_fp, c_int64, c_float, c_float, c_fp, c_fp, c_void_p]),
    'sda_pairwise_dist': (c_int, [c_fp, c_int, c_fp, c_int, c_int64, c_int, c_fp, c_void_p]),
    'sda_mmd_kernel_sums': (c_int, [c_fp, c_int64, c_void_p, c_int, c_void_p]),
    'sda_assignment_cost': (c_int, [c_void_p, c_int, c_void_p, c_void_p]),
    'sda_transport_cost': (c_int, [c_void_p, c_int, c_int, c_void_p]),
    'sda_assignment_auction': (c_int, [c_fp, c_int, c_int, ctypes.c_double, c_int64, c_fp, c_fp, c_fp, c_fp, c_fp, c_fp, c_void_p]),
    'sda_conv3d': (c_int, [POINTER(Conv3dDesc), c_void_p]),
    'sda_conv3d_packed_floats': (c_int64, [c_int, c_int, c_int, c_int, c_int, c_int]),
    'sda_pack_conv3d_weight': (c_int, [c_fp, c_int, c_int, c_int, c_int, c_int, c_int, c_fp, c_void_p]),
    'sda_chain_advance': (c_int, [POINTER(ChainAdv), c_void_p]),
    'sda_chain_log_prob': (c_int, [POINTER(ChainModel), c_fp, c_int, c_int, c_int64, c_int64, c_fp, c_void_p]),
    'sda_bpf_logweights': (c_int, [c_fp, c_int, c_int64, c_int, POINTER(ChainObs), c_fp, c_fp, c_void_p]),
    'sda_bpf_logweights_blocks': (c_int, [c_int]),
    'sda_bpf_cdf': (c_int, [c_fp, c_int, c_fp, c_int, c_fp, c_fp, c_fp, c_void_p]),
    'sda_bpf_resample': (c_int, [c_fp, c_int, c_uint64, c_int64, c_fp, c_void_p]),
    'sda_bpf_traceback': (c_int, [c_fp, c_int64, c_int64, c_fp, c_int, c_int, c_int, c_int, c_fp, c_void_p]),
    'sda_chain_advance_vjp': (c_int, [POINTER(ChainVjp), c_void_p]),
    'sda_chain_log_prob_grad': (c_int, [POINTER(ChainModel), c_fp, c_int, c_int, c_int64, c_int64, c_fp, c_fp, c_void_p]),
    'sda_pool3d_sum': (c_int, [c_fp, c_int64, c_int, c_int, c_int, c_int, c_int, c_int, c_fp, c_void_p]),
    'sda_kflow_serves': (c_int, [c_int]),
    'sda_kflow_work_floats': (c_int64, [c_int, c_int]),
    'sda_kflow_explicit': (c_int, [POINTER(KflowModel), c_fp, c_int64, c_int, c_fp, c_void_p]),
    'sda_kflow_hartley': (c_int, [c_fp, c_int, c_fp, c_int64, c_int, c_int, c_fp, c_fp, c_void_p]),
    'sda_kflow_project': (c_int, [POINTER(KflowModel), c_fp, c_int64, c_int, c_fp, c_int64, c_fp, c_void_p]),
    'sda_kflow_advance': (c_int, [POINTER(KflowModel), c_fp, c_int64, c_int, c_int, c_int, c_fp, c_int64, c_fp, c_void_p]),
    # the adjoint of the flow; its own prefix: tests/test_kflow_host.py pins the list of sda_kflow_* entries
    'sda_kfvjp_work_floats': (c_int64, [c_int, c_int, c_int]),
    'sda_kfvjp_explicit': (c_int, [POINTER(KflowModel), c_fp, c_int64, c_fp, c_int64, c_int, c_fp, c_void_p]),
    'sda_kfvjp_transition': (c_int, [POINTER(KflowModel), c_fp, c_int64, c_fp, c_int64, c_int, c_fp, c_fp, c_void_p]),
    # linear-Gaussian state space (csrc/lgss.hip); sda_lgss_tables takes a HOST table
    'sda_lgss_advance': (c_int, [POINTER(LgssModel), c_fp, c_int64, c_int, c_int, c_int, c_fp, c_int64, c_int64, c_uint64, c_int64, c_int64,
                                 c_void_p]),
    'sda_lgss_table_doubles': (c_int64, [c_int, c_int, c_int]),
    'sda_lgss_tables': (c_int, [POINTER(LgssModel64), c_int, c_int, c_void_p]),
    'sda_lgss_filter': (c_int, [POINTER(LgssModel64), c_fp, c_int, c_int, c_fp, c_int, c_fp, c_fp, c_void_p]),
    'sda_lgss_sample': (c_int, [POINTER(LgssModel64), c_fp, c_fp, c_int, c_int, c_int, c_uint64, c_int64, c_int64, c_fp, c_void_p]),
    'sda_lgss_score_doubles': (c_int64, [c_int, c_int, c_int]),
    'sda_lgss_score_factor': (c_int, [c_int, c_int, c_fp, c_fp, c_fp, c_void_p]),
    'sda_lgss_score': (c_int, [c_int, c_int, c_fp, c_fp, c_fp, c_fp, c_int, c_int, c_fp, c_fp, c_void_p]),
    # ensemble Kalman smoother (csrc/enks.hip)
    'sda_enks_gain': (c_int, [c_fp, c_int, c_int64, c_int, POINTER(ChainObs), c_float, c_uint64, c_int64, c_fp, c_fp, c_fp, c_fp, c_void_p]),
    'sda_enks_update': (c_int, [c_fp, c_int64, c_int64, c_int, c_int, c_int, c_int, c_float, c_fp, c_fp, c_void_p]),
    # its ensemble-space form for wide states (csrc/enks_wide.hip)
    'sda_enkw_gram_doubles': (c_int64, [c_int, c_int]),
    'sda_enkw_prepare': (c_int, [c_fp, c_int, c_int, c_fp, c_float, c_uint64, c_int64, c_fp, c_fp, c_fp, c_void_p]),
    'sda_enkw_gram': (c_int, [c_fp, c_fp, c_int, c_int, c_fp, c_void_p]),
    'sda_enkw_solve': (c_int, [c_fp, c_int, c_int, c_float, c_fp, c_fp, c_fp, c_void_p]),
    'sda_enkw_transform': (c_int, [c_fp, c_int64, c_int64, c_int, c_int, c_int64, c_fp, c_float, c_int, c_void_p]),
    # its domain-localised form for grid states (csrc/enks_local.hip)
    'sda_enkl_pack': (c_int, [c_fp, c_fp, c_int, c_int, c_fp, c_void_p]),
    'sda_enkl_weights': (c_int, [c_fp, c_int, c_int, c_fp, c_fp, c_fp, c_int, c_float, c_fp, c_fp, c_fp, c_void_p]),
    'sda_enkl_transform': (c_int, [c_fp, c_int64, c_int64, c_int, c_int, c_int, c_int, c_int, c_int, c_int, c_fp, c_fp, c_void_p]),
}

_lib = None


class SdaHipError(RuntimeError):
    pass


def load():
    """Load libsda_hip.so and bind every declared symbol.  Raises (never falls back) if anything is missing."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise SdaHipError(
            f'{LIB_PATH} not found: the HIP extension is not built. Run `python -m sda_amd.build` '
            f'(or __graft_entry__.build()). sda_amd has no CPU fallback.')
    if os.environ.get('SDA_HIP_LIB'):
        import warnings
        warnings.warn(f'sda_amd: kernel library overridden by SDA_HIP_LIB={LIB_PATH} (a tooling build; bench.py records it as '
                      f'`kernel_library_override`)')
    lib = ctypes.CDLL(LIB_PATH)
    for name, (res, args) in SIGNATURES.items():
        try:
            fn = getattr(lib, name)
        except AttributeError as e:
            raise SdaHipError(f'libsda_hip.so does not export {name}') from e
        fn.restype = res
        fn.argtypes = args
    _lib = lib
    return lib


def check(rc, what):
    if rc != 0:
        if rc < 0:
            msg = {-1: 'bad argument', -2: 'unsupported shape', -3: 'tile exceeds LDS'}.get(rc, 'error')
            raise SdaHipError(f'{what}: {msg} (SDA_E {rc})')
        raise SdaHipError(f'{what}: HIP launch error {rc}')
