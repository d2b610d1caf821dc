"""ctypes binding of libmdgrad_hip.so (the C ABI declared in include/mdgrad_hip.h).

There is NO fallback: if the HIP library is missing this module raises, and every hot-path
op in the package goes through it.  PyTorch is used only for device memory, streams and
autograd bookkeeping; pointers handed to the library are `tensor.data_ptr()`.
"""
import ctypes as C
import os

import torch

_HERE = os.path.dirname(os.path.abspath(__file__))
# (MDG_LIB: another build of the same library, e.g. a compile-time variant of one kernel file for an A/B run -- tools/variants.sh)
LIB_PATH = os.environ.get("MDG_LIB") or os.path.join(_HERE, "lib", "libmdgrad_hip.so")

MAX_TERMS, MAX_THETA, MAX_CHAINS = 4, 3, 16
PAIR_LJ, PAIR_MORSE, PAIR_BUCK, PAIR_YUKAWA = 0, 1, 2, 3


class MdgPairTerm(C.Structure):
    _fields_ = [("kind", C.c_int32), ("p", C.c_int32), ("q", C.c_int32), ("c", C.c_float),
                ("a", C.c_float), ("phi", C.c_float), ("cutoff", C.c_float),
                ("theta_off", C.c_int32), ("n_theta", C.c_int32), ("reserved", C.c_int32),
                ("mask", C.c_void_p)]


class MdgTerms(C.Structure):
    _fields_ = [("n_terms", C.c_int32), ("n_theta_total", C.c_int32), ("t", MdgPairTerm * MAX_TERMS)]


class MdgCell(C.Structure):
    _fields_ = [("h", C.c_float * 9), ("inv", C.c_float * 9), ("diag", C.c_int32)]


class MdgTrajParams(C.Structure):
    _fields_ = [("n_rep", C.c_int32), ("n_atoms", C.c_int32), ("n_frames", C.c_int32),
                ("n_chains", C.c_int32), ("ensemble", C.c_int32), ("block", C.c_int32),
                ("T", C.c_float), ("n_dof", C.c_float), ("Q", C.c_float * MAX_CHAINS)]


class MdgRdfFuse(C.Structure):
    """Fused RDF observable of the wave-per-replica trajectory kernels (include/mdgrad_hip.h)."""
    _fields_ = [("mu", C.c_void_p), ("nbins", C.c_int32), ("coeff", C.c_float), ("mu0", C.c_float), ("spacing", C.c_float),
                ("cutoff", C.c_float), ("frame_start", C.c_int32), ("frame_stride", C.c_int32)]


class MdgFilterNet(C.Structure):
    """Host struct of device pointers describing one SchNet filter network (include/mdgrad_hip.h)."""
    _fields_ = [("mu", C.c_void_p), ("coef", C.c_void_p), ("W1", C.c_void_p), ("b1", C.c_void_p),
                ("W2", C.c_void_p), ("b2", C.c_void_p), ("n_gauss", C.c_int32), ("n_filters", C.c_int32)]


class MdgGradJob(C.Structure):
    """One reduction of mdg_grad_jobs (include/mdgrad_hip.h)."""
    _fields_ = [("A", C.c_void_p), ("B", C.c_void_p), ("A2", C.c_void_p), ("B2", C.c_void_p), ("row_map", C.c_void_p),
                ("rows", C.c_int64), ("m", C.c_int32), ("n", C.c_int32), ("kind", C.c_int32), ("pad_", C.c_int32),
                ("out_off", C.c_int64)]


GRAD_ATB, GRAD_COLSUM, GRAD_AXPY, GRAD_JOBS_MAX = 0, 1, 2, 32


class MdgCoulombConsts(C.Structure):
    """Constants of the damped shifted-force Coulomb sum, prepared in double (include/mdgrad_hip.h K20)."""
    _fields_ = [(n, C.c_double) for n in ("alpha", "rc", "c0", "c1", "g0", "alpha2", "conversion", "self_s")]


class MdgSWConsts(C.Structure):
    """Constants of the Stillinger-Weber term and host copies of (epsilon, sigma, lam) (include/mdgrad_hip.h K23)."""
    _fields_ = [(n, C.c_double) for n in ("epsilon", "sigma", "lam", "a", "gamma", "cos0", "A", "B")] + \
               [("p", C.c_int32), ("q", C.c_int32)]


class MdgEAMConsts(C.Structure):
    """Constants of the Sutton-Chen term and host copies of (epsilon, a, c) (include/mdgrad_hip.h K24)."""
    _fields_ = [(n, C.c_double) for n in ("epsilon", "a", "c", "rc")] + \
               [(n, C.c_int32) for n in ("n", "m", "shift", "pad_")]


class MdgEAMTableConsts(C.Structure):
    """The grids of the tabulated embedded-atom term (include/mdgrad_hip.h K27)."""
    _fields_ = [(n, C.c_double) for n in ("r_min", "h_r", "rc", "rho_min", "h_rho")] + \
               [(n, C.c_int32) for n in ("n_species", "n_r", "n_rho", "pin_cutoff")]


class MdgTersoffConsts(C.Structure):
    """Constants of the Tersoff term and host copies of (A, B, h) (include/mdgrad_hip.h K25)."""
    _fields_ = [(n, C.c_double) for n in ("A", "B", "lam1", "lam2", "beta", "n", "c", "d", "h", "R", "D", "lam3", "gamma")] + \
               [(n, C.c_int32) for n in ("m", "pad_")]


class MdgChainStage(C.Structure):
    """One Dense stage of mdg_row_chain (include/mdgrad_hip.h)."""
    _fields_ = [(n, C.c_void_p) for n in ("W", "bias", "in0", "in1", "res0", "res1", "aux0", "aux1", "out0", "out1", "sig",
                                          "pre0", "pre1", "out0_h", "out1_h")] + \
               [(n, C.c_int32) for n in ("K", "M", "trans", "act", "mode", "pad_")]


SCHNET_MAX_LAYERS = 8


class MdgSchnetLayer(C.Structure):
    """One interaction block of MdgSchnetPlan (include/mdgrad_hip.h)."""
    _fields_ = [("filt", MdgFilterNet)] + [(n, C.c_void_p) for n in ("Wn", "bn", "U1", "c1", "U2", "c2")] + \
               [("off_" + n, C.c_int64) for n in ("W1", "b1", "W2", "b2", "Wn", "bn", "U1", "c1", "U2", "c2")] + \
               [(n, C.c_int32) for n in ("bf16", "bf16_rev", "rows16", "b2col")]


class MdgSchnetPlan(C.Structure):
    """A SchNet network + topology + workspace for mdg_schnet_force / mdg_schnet_force_vjp (include/mdgrad_hip.h)."""
    _fields_ = [(n, C.c_int32) for n in ("n_atoms", "n_layers", "n_atom_basis", "n_readout")] + \
               [("layer", MdgSchnetLayer * SCHNET_MAX_LAYERS)] + [(n, C.c_void_p) for n in ("L1", "l1", "L2")] + \
               [(n, C.c_int64) for n in ("off_L1", "off_l1", "off_L2", "off_embed")] + \
               [(n, C.c_void_p) for n in ("r0", "h0", "h0_16", "onehot", "uniq")] + [("n_species", C.c_int32), ("masked", C.c_int32)] + \
               [("nbr", C.c_void_p), ("offsets", C.c_void_p), ("n_edges", C.c_int64)] + \
               [(n, C.c_void_p) for n in ("col", "eid", "cnt", "n_valid")] + [("max_nbr", C.c_int32), ("cutoff", C.c_float)] + \
               [("cell", MdgCell), ("ws", C.c_void_p), ("ws_floats", C.c_int64), ("stash", C.c_int32), ("chain_x3", C.c_int32)]


CHAIN_NONE, CHAIN_MUL, CHAIN_HEAD, CHAIN_SSP_BWD, CHAIN_MAX_STAGES, CHAIN_MAX_WIDTH = 0, 1, 2, 3, 8, 512
BONDED_BOND, BONDED_ANGLE = 0, 1                 # include/mdgrad_hip.h MDG_BONDED_*
CFCONV_BF16, CFCONV_ROWS16 = 1, 2                # include/mdgrad_hip.h MDG_CFCONV_*

P = C.c_void_p
_SIGNATURES = {
    "mdg_last_error": (C.c_char_p, []),
    "mdg_version": (C.c_int, []),
    "mdg_nbr_build_dense": (C.c_int, [P, C.c_int, C.POINTER(MdgCell), C.c_float, P, P, P, P, C.c_int, P, P]),
    "mdg_nbr_build_dense_groups": (C.c_int, [P, C.c_int, C.c_int, C.POINTER(MdgCell), C.c_float, P, P, P, P,
                                             C.c_int, P, P]),
    "mdg_nbr_cell_bins": (C.c_int, [C.POINTER(MdgCell), C.c_float, C.POINTER(C.c_int32)]),
    "mdg_nbr_cell_scratch": (C.c_int64, [C.c_int, C.POINTER(MdgCell), C.c_float]),
    "mdg_nbr_build_cell":(C.c_int, [P, C.c_int, C.POINTER(MdgCell), C.c_float, P, P, P, P, C.c_int, P, P, P]),
    "mdg_nbr_cell_scratch_groups": (C.c_int64, [C.c_int, C.c_int, C.POINTER(MdgCell), C.c_float]),
    "mdg_nbr_build_cell_groups": (C.c_int, [P, C.c_int, C.c_int, C.POINTER(MdgCell), C.c_float, P, P, P, P, C.c_int,
                                            P, P, P]),
    "mdg_nbr_half_count": (C.c_int, [P, P, C.c_int, C.c_int, P, P]),
    "mdg_nbr_half_fill": (C.c_int, [P, P, P, P, C.c_int, C.c_int, P, P, P, P]),
    "mdg_nbr_half_fill_padded": (C.c_int, [P, P, P, P, C.c_int, C.c_int, C.c_int64, C.c_float, P, P, P, P, P, P]),
    "mdg_nbr_verlet_rebuild": (C.c_int, [P, C.c_int, C.c_int, C.POINTER(MdgCell), C.c_float, C.c_float, P, C.c_int, P, P, P,
                                         C.c_int, C.c_int64, C.c_float, P, P, P, P, P, P, P, P, P, P]),
    "mdg_edge_geom_prepare": (C.c_int, [P, P, P, P, C.c_int64, C.POINTER(MdgCell), C.c_float, P, P, P, P, P, C.c_int64, P]),
    "mdg_edge_geom_masked": (C.c_int, [P, P, P, P, C.c_int64, C.POINTER(MdgCell), C.c_float, P, P, P, P, P]),
    "mdg_pair_partial_size": (C.c_int64, [C.c_int]),
    "mdg_pair_eval_ell": (C.c_int, [P, C.c_int, C.POINTER(MdgCell), P, P, P, C.c_int,
                                    C.POINTER(MdgPairTerm), P, P, P, P, P, P, P, P, P]),
    "mdg_pair_eval_ell_into": (C.c_int, [P, C.c_int, C.POINTER(MdgCell), P, P, P, C.c_int,
                                         C.POINTER(MdgPairTerm), P, P, P, P, P, P, P, P, C.c_float, C.c_int, P]),
    "mdg_traj_fwd_small": (C.c_int, [C.POINTER(MdgTrajParams), C.POINTER(MdgCell), C.POINTER(MdgTerms),
                                     P, P, P, P, P, P, P, P, P, P, P]),
    "mdg_traj_adj_small": (C.c_int, [C.POINTER(MdgTrajParams), C.POINTER(MdgCell), C.POINTER(MdgTerms),
                                     P, P, P, P, P, P, P, P, P, P, P, P, P, P]),
    "mdg_traj_ring_taken": (C.c_int, [C.POINTER(MdgTrajParams), C.POINTER(MdgCell), C.POINTER(MdgTerms)]),
    "mdg_traj_small_fits": (C.c_int, [C.c_int, C.c_int]),
    "mdg_min_image_fused_inv": (C.c_int, [C.c_float, C.c_float, C.POINTER(C.c_float)]),
    "mdg_traj_ring_fused_image": (C.c_int, [C.POINTER(MdgTrajParams), C.POINTER(MdgCell), C.POINTER(MdgTerms)]),
    "mdg_traj_fwd_small_ft": (C.c_int, [C.POINTER(MdgTrajParams), C.POINTER(MdgCell), C.POINTER(MdgTerms),
                                        P, P, P, P, P, P, P, P, P, P, P, P]),
    "mdg_traj_adj_small_ft": (C.c_int, [C.POINTER(MdgTrajParams), C.POINTER(MdgCell), C.POINTER(MdgTerms),
                                        P, P, P, P, P, P, P, P, P, P, P, P, P, P, P]),
    "mdg_traj_fwd_small_rdf_ft": (C.c_int, [C.POINTER(MdgTrajParams), C.POINTER(MdgCell), C.POINTER(MdgTerms),
                                            P, P, P, P, P, P, P, P, P, P, P, C.POINTER(MdgRdfFuse), P, P]),
    "mdg_traj_adj_small_rdf_ft": (C.c_int, [C.POINTER(MdgTrajParams), C.POINTER(MdgCell), C.POINTER(MdgTerms),
                                            P, P, P, P, P, P, P, P, P, P, P, P, P, P, C.POINTER(MdgRdfFuse), P, P]),
    "mdg_traj_rdf_supported": (C.c_int, [C.POINTER(MdgTrajParams), C.POINTER(MdgCell), C.POINTER(MdgTerms),
                                         C.POINTER(MdgRdfFuse)]),
    "mdg_traj_fwd_small_rdf": (C.c_int, [C.POINTER(MdgTrajParams), C.POINTER(MdgCell), C.POINTER(MdgTerms),
                                         P, P, P, P, P, P, P, P, P, P, C.POINTER(MdgRdfFuse), P, P]),
    "mdg_traj_adj_small_rdf": (C.c_int, [C.POINTER(MdgTrajParams), C.POINTER(MdgCell), C.POINTER(MdgTerms),
                                         P, P, P, P, P, P, P, P, P, P, P, P, P, C.POINTER(MdgRdfFuse), P, P]),
    "mdg_traj_large_workspace": (C.c_int64, [C.c_int, C.c_int, C.c_int, C.c_int]),
    "mdg_traj_large_list_builds": (C.c_int, [P, C.c_int, C.c_int, C.c_int, C.c_int, P, P]),
    "mdg_traj_fwd_large": (C.c_int, [C.POINTER(MdgTrajParams), C.POINTER(MdgCell), C.POINTER(MdgTerms),
                                     P, P, P, P, P, P, P, P, P, P, P, P]),
    "mdg_traj_adj_large": (C.c_int, [C.POINTER(MdgTrajParams), C.POINTER(MdgCell), C.POINTER(MdgTerms),
                                     P, P, P, P, P, P, P, P, P, P, P, P, P, P, P]),
    "mdg_traj_large_stale_words": (C.c_int64, [C.c_int, C.c_int]),
    "mdg_traj_fwd_large_stale": (C.c_int, [C.POINTER(MdgTrajParams), C.POINTER(MdgCell), C.POINTER(MdgTerms),
                                           P, P, P, P, P, P, P, P, P, P, P, C.c_int, C.c_int64, P, P]),
    "mdg_traj_adj_large_stale": (C.c_int, [C.POINTER(MdgTrajParams), C.POINTER(MdgCell), C.POINTER(MdgTerms),
                                           P, P, P, P, P, P, P, P, P, P, P, P, P, P, P, C.c_int, C.c_int64, P, P]),
    "mdg_rdf_partial_size": (C.c_int64, [C.c_int, C.c_int, C.c_int]),
    "mdg_rdf_fwd": (C.c_int, [P, C.c_int, C.c_int, C.POINTER(MdgCell), C.c_float, P, P, C.c_float,
                              C.c_int, P, P, P]),
    "mdg_rdf_fwd_uniform": (C.c_int, [P, C.c_int, C.c_int, C.POINTER(MdgCell), C.c_float, P, P, C.c_float, C.c_float,
                                      C.c_int, P, P, P]),
    "mdg_rdf_fwd_variant": (C.c_int, [C.c_int, C.c_int, C.c_int, C.c_float, C.c_float, C.c_int, C.c_int, C.POINTER(C.c_int32)]),
    "mdg_rdf_bwd_variant": (C.c_int, [C.c_int, C.c_int, C.c_int, C.c_float, C.c_float, C.c_int, C.c_int, C.POINTER(C.c_int32)]),
    "mdg_rdf_fine_grid": (C.c_int, [C.c_float, C.c_float, C.c_int, C.POINTER(C.c_int32), C.POINTER(C.c_float),
                                    C.POINTER(C.c_float), C.POINTER(C.c_int32)]),
    "mdg_rdf_ell_supported": (C.c_int, [C.c_float, C.c_float, C.c_int]),
    "mdg_rdf_fwd_ell": (C.c_int, [P, C.c_int64, C.POINTER(MdgCell), P, P, P, C.c_int, P, C.c_float, C.c_float, C.c_int, P, P]),
    "mdg_rdf_cell_supported": (C.c_int, [C.c_int, C.POINTER(MdgCell), C.c_float]),
    "mdg_rdf_cell_scratch": (C.c_int64, [C.c_int, C.c_int, C.POINTER(MdgCell), C.c_float]),
    "mdg_rdf_fwd_cell": (C.c_int, [P, C.c_int, C.c_int, C.POINTER(MdgCell), C.c_float, P, C.c_float, C.c_float, C.c_int,
                                   P, P, P]),
    "mdg_rdf_bwd_cell": (C.c_int, [C.c_int, C.c_int, C.POINTER(MdgCell), C.c_float, C.POINTER(MdgPairTerm), P, P, P, P]),
    "mdg_rdf_bwd": (C.c_int, [P, C.c_int, C.c_int, C.POINTER(MdgCell), C.c_float, P, P, C.c_float,
                              C.c_int, P, P, P]),
    "mdg_rdf_bwd_uniform": (C.c_int, [P, C.c_int, C.c_int, C.POINTER(MdgCell), C.c_float, P, P, C.c_float, C.c_float,
                                      C.c_int, P, P, P]),
    "mdg_nhc_rhs": (C.c_int, [P, P, P, P, P, P, C.c_float, C.c_int, C.c_int, C.c_int, P, P, P]),
    "mdg_nhc_vjp": (C.c_int, [P, P, P, P, P, P, P, C.c_int, C.c_int, C.c_int, P, P, P]),
    "mdg_row_chain": (C.c_int, [P, C.c_int, C.c_int, C.c_int, P]),      # (MdgChainStage*: an array object or a raw address)
    "mdg_nhv_scratch_floats": (C.c_int64, [C.c_int, C.c_int]),
    "mdg_nhv_kick": (C.c_int, [P, P, P, P, P, P, P, C.c_float, P, P, C.c_int, C.c_int, C.c_int, P, P, P, P, P]),
    "mdg_nhv_finish": (C.c_int, [P, P, P, P, P, P, P, P, P, P, P, C.c_float, P, P, C.c_int, C.c_int, C.c_int, C.c_int, P, P, P, P,
                                 P]),
    "mdg_nhv_adj_pre": (C.c_int, [P, P, P, P, P, P, C.c_int, C.c_int, C.c_int, P, P, P, P, P]),
    "mdg_nhv_adj_mid": (C.c_int, [P, P, P, P, P, P, P, P, P, P, P, C.c_float, P, P, C.c_int, C.c_int, C.c_int,
                                  P, P, P, P, P, P, P, P, P]),
    "mdg_nhv_adj_end": (C.c_int, [P, P, P, P, P, P, P, P, P, P, C.c_int, P, P, P, C.c_int, C.c_int, C.c_int, P, P, P, P, P]),
    "mdg_lgv_blocks": (C.c_int, [C.c_int]),
    "mdg_lgv_noise": (C.c_int, [P, C.c_int64, C.c_int, P, P]),
    "mdg_lgv_kick": (C.c_int, [P, P, P, P, P, P, P, P, P, C.c_int, P, P, P]),
    "mdg_lgv_finish": (C.c_int, [P, P, P, P, P, P, P, P, P, C.c_int, C.c_int, P, P, P, P]),
    "mdg_lgv_adj_pre": (C.c_int, [P, P, P, P, P, C.c_int, P, P, P]),
    "mdg_lgv_adj_step": (C.c_int, [P, P, P, P, P, P, P, P, P, C.c_int, P, P, P, C.c_int, C.c_int, P, P, P, P, P, P, P]),
    "mdg_lgv_gamma_sum": (C.c_int, [P, C.c_int, P, P]),
    "mdg_edge_diff": (C.c_int, [P, P, C.c_int64, C.c_int, P, P]),
    "mdg_edge_scatter": (C.c_int, [P, P, P, P, C.c_int, C.c_int, C.c_int, P, P]),
    "mdg_cfconv_agg": (C.c_int, [P, P, P, P, P, C.c_int, C.c_int, C.c_int, P, P]),
    "mdg_edge_prod": (C.c_int, [P, P, P, C.c_int64, C.c_int, P, P]),
    "mdg_smear": (C.c_int, [P, P, P, C.c_int64, C.c_int, P, P, P]),
    "mdg_ssp": (C.c_int, [P, C.c_int64, P, P, P]),
    "mdg_mul_row": (C.c_int, [P, P, P, C.c_int64, C.c_int, P, P]),
    "mdg_ssp_dual_bwd": (C.c_int, [P, P, P, P, C.c_int64, P, P, P]),
    "mdg_ssp_dual_bwd_t": (C.c_int, [P, P, P, P, C.c_int64, P, P, P]),
    "mdg_readout_head": (C.c_int, [P, P, P, C.c_int64, C.c_int, P, P, P]),
    "mdg_smear_bwd": (C.c_int, [P, P, P, P, P, P, C.c_int64, C.c_int, P, P, P]),
    "mdg_atb_workspace": (C.c_int64, [C.c_int64, C.c_int, C.c_int]),
    "mdg_atb": (C.c_int, [P, P, C.c_int64, C.c_int, C.c_int, P, P, P]),
    "mdg_atb2": (C.c_int, [P, P, P, P, C.c_int64, C.c_int, C.c_int, P, P, P]),
    "mdg_grad_jobs_workspace": (C.c_int64, [P, C.c_int]),
    "mdg_grad_jobs": (C.c_int, [P, C.c_int, P, C.c_float, P, P, C.c_int, P, P]),
    "mdg_vacf_workspace": (C.c_int64, [C.c_int]),
    "mdg_vacf_fwd": (C.c_int, [P, C.c_int, C.c_int64, C.c_int, P, P, P]),
    "mdg_vacf_bwd": (C.c_int, [P, P, C.c_int, C.c_int64, C.c_int, P, P]),
    "mdg_temperature": (C.c_int, [P, P, C.c_int, C.c_int, C.c_float, P, P]),
    "mdg_cfconv_supported": (C.c_int, [C.c_int, C.c_int]),
    "mdg_edge_geom": (C.c_int, [P, P, P, P, C.c_int64, P, P, P, P, P]),
    "mdg_edge_geom_bwd": (C.c_int, [P, P, P, P, P, P, P, P, P, C.c_int, C.c_int, P, P, P]),
    "mdg_cfconv_fwd": (C.c_int, [C.POINTER(MdgFilterNet), P, P, P, P, P, P, P, C.c_int, C.c_int, P, P, P, P, P]),
    "mdg_cfconv_fwd_bf16": (C.c_int, [C.POINTER(MdgFilterNet), P, P, P, P, P, P, P, C.c_int, C.c_int, P, P, P, P, P]),
    "mdg_cfconv_bwd_workspace": (C.c_int64, [C.c_int, C.c_int, C.c_int64]),
    "mdg_cfconv_bwd": (C.c_int, [C.POINTER(MdgFilterNet), P, P, P, C.c_int64, P, P, P, P, P, P, P, P, P, P, P, P]),
    "mdg_cfconv_bwd_bf16": (C.c_int, [C.POINTER(MdgFilterNet), P, P, P, C.c_int64, P, P, P, P, P, P, P, P, P, P, P, P]),
    "mdg_cfconv_bwd_smear": (C.c_int, [C.POINTER(MdgFilterNet), P, P, P, C.c_int64, P, P, P, P, P, P, P, P, P, P, P, P, P,
                                       C.c_int, P]),
    "mdg_cfconv_rows16_supported": (C.c_int, [C.c_int, C.c_int]),
    "mdg_cfconv_fwd_rows16": (C.c_int, [C.POINTER(MdgFilterNet), P, P, P, P, P, P, P, C.c_int, C.c_int, P, P, P, P, P]),
    "mdg_cfconv_bwd_rows16": (C.c_int, [C.POINTER(MdgFilterNet), P, P, P, C.c_int64, C.c_int, P, P, P, P, P, P, P, P, P, P, P, P,
                                        P, P]),
    "mdg_rows_to_bf16": (C.c_int, [P, C.c_int64, C.c_int, C.c_int, P, P]),
    "mdg_cfconv_stash_width": (C.c_int, [C.c_int]),
    "mdg_cfconv_filter_stash": (C.c_int, [C.POINTER(MdgFilterNet), P, P, C.c_int64, P, P, P, P]),
    "mdg_cfconv_fwd_stashed": (C.c_int, [C.POINTER(MdgFilterNet), P, P, P, P, P, P, P, P, C.c_int, C.c_int, P, P, C.c_int, P]),
    "mdg_cfconv_bias_column": (C.c_int, [C.c_int]),
    "mdg_cfconv_bwd_theta": (C.c_int, [C.POINTER(MdgFilterNet), P, P, P, C.c_int64, C.c_int, P, P, P, P, P, P, P, P, P, P, P, P,
                                       P, P, C.c_int, P]),
    "mdg_dense": (C.c_int, [P, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, P, P, P, P, P, P, P, P, P, P]),
    "mdg_cfconv_filter": (C.c_int, [P, C.c_int64, P, P, C.c_int, P, P, P, P, C.c_int, P, P]),
    "mdg_cfconv_filter_bf16": (C.c_int, [P, C.c_int64, P, P, C.c_int, P, P, P, P, C.c_int, P, P]),
    "mdg_traj_stale_words": (C.c_int64, [C.c_int, C.c_int]),
    "mdg_traj_fwd_small_stale": (C.c_int, [C.POINTER(MdgTrajParams), C.POINTER(MdgCell), C.POINTER(MdgTerms), P, P, P, P, P, P,
                                           P, P, P, P, C.c_int, C.c_int64, P, P]),
    "mdg_traj_adj_small_stale": (C.c_int, [C.POINTER(MdgTrajParams), C.POINTER(MdgCell), C.POINTER(MdgTerms), P, P, P, P, P, P,
                                           P, P, P, P, P, P, P, C.c_int, C.c_int64, P, P]),
    "mdg_schnet_plan_sizeof": (C.c_int64, []),
    "mdg_schnet_workspace": (C.c_int64, [C.POINTER(MdgSchnetPlan), C.c_int, C.c_int]),
    "mdg_schnet_force": (C.c_int, [C.POINTER(MdgSchnetPlan), P, P, P, P]),
    "mdg_schnet_force_vjp": (C.c_int, [C.POINTER(MdgSchnetPlan), P, P, P, P, P, C.c_float, P, P, P, P]),
    "mdg_adf_partial_size": (C.c_int64, [C.c_int, C.c_int, C.c_int, C.c_int]),
    "mdg_adf_fwd": (C.c_int, [P, C.c_int, C.c_int, C.POINTER(MdgCell), C.c_float, P, P, C.c_int, P, C.c_float, C.c_float,
                              C.c_int, P, P, P]),
    "mdg_adf_bwd": (C.c_int, [P, C.c_int, C.c_int, C.POINTER(MdgCell), C.c_float, P, P, C.c_int, P, C.c_float, C.c_float,
                              C.c_int, P, P, P]),
    "mdg_adf_frames_fwd": (C.c_int, [P, C.c_int, C.c_int, C.POINTER(MdgCell), C.c_float, P, P, C.c_int, P, C.c_float, C.c_float,
                                     C.c_int, P, P]),
    "mdg_adf_frames_bwd": (C.c_int, [P, C.c_int, C.c_int, C.POINTER(MdgCell), C.c_float, P, P, C.c_int, P, C.c_float, C.c_float,
                                     C.c_int, P, P, P]),
    "mdg_bond_order_components": (C.c_int, [P, C.c_int]),
    "mdg_bond_order_fwd": (C.c_int, [P, C.c_int, C.c_int, C.POINTER(MdgCell), C.c_float, C.c_float, P, P, C.c_int, P, C.c_int, P, P,
                                     P]),
    "mdg_bond_order_bwd": (C.c_int, [P, C.c_int, C.c_int, C.POINTER(MdgCell), C.c_float, C.c_float, P, P, C.c_int, P, C.c_int, P, P,
                                     P, P]),
    "mdg_virial_workspace": (C.c_int64, [C.c_int, C.c_int, C.c_int]),
    "mdg_virial_fwd": (C.c_int, [P, C.c_int, C.c_int, C.POINTER(MdgCell), C.POINTER(MdgTerms), P, P, P, P]),
    "mdg_virial_bwd": (C.c_int, [P, C.c_int, C.c_int, C.POINTER(MdgCell), C.POINTER(MdgTerms), P, P, P, P, P, P]),
    "mdg_energy_frames_workspace": (C.c_int64, [C.c_int, C.c_int, C.c_int]),
    "mdg_energy_frames_fwd": (C.c_int, [P, C.c_int, C.c_int, C.POINTER(MdgCell), C.POINTER(MdgTerms), P, P, P, P]),
    "mdg_energy_frames_bwd": (C.c_int, [P, C.c_int, C.c_int, C.POINTER(MdgCell), C.POINTER(MdgTerms), P, P, P, P, P, P]),
    "mdg_energy_table_workspace": (C.c_int64, [C.c_int, C.c_int, C.c_int]),
    "mdg_energy_table_fwd": (C.c_int, [P, C.c_int, C.c_int, C.POINTER(MdgCell), P, C.c_int, C.c_float, C.c_float, C.c_float, P,
                                       P, P, P, P]),
    "mdg_energy_table_bwd": (C.c_int, [P, C.c_int, C.c_int, C.POINTER(MdgCell), P, C.c_int, C.c_float, C.c_float, C.c_float, P,
                                       P, P, P, P, P]),
    "mdg_rdf_frames_fwd": (C.c_int, [P, C.c_int, C.c_int, C.POINTER(MdgCell), C.c_float, P, P, C.c_float, C.c_float, C.c_int, P,
                                     P]),
    "mdg_rdf_frames_bwd": (C.c_int, [P, C.c_int, C.c_int, C.POINTER(MdgCell), C.c_float, P, P, C.c_float, C.c_float, C.c_int, P,
                                     P, P]),
    "mdg_sk_workspace": (C.c_int64, [C.c_int, C.c_int, C.c_int]),
    "mdg_sk_fwd": (C.c_int, [P, C.c_int, C.c_int, C.POINTER(MdgCell), P, C.c_float, P, C.c_int, P, C.c_int, P, P, P]),
    "mdg_sk_bwd": (C.c_int, [P, C.c_int, C.c_int, C.POINTER(MdgCell), P, C.c_float, P, C.c_int, P, C.c_int, P, P, P, P]),
    "mdg_msd_workspace": (C.c_int64, [C.c_int, C.c_int, C.c_int, C.c_int, C.c_int]),
    "mdg_msd_fwd": (C.c_int, [P, C.c_int, C.c_int, C.c_int, C.c_int, P, C.c_int, C.c_int, P, P, P, P]),
    "mdg_msd_bwd": (C.c_int, [P, C.c_int, C.c_int, C.c_int, C.c_int, P, C.c_int, C.c_int, P, P, P, P, P]),
    "mdg_msd_tile_atoms": (C.c_int, []),
    "mdg_msd_window": (C.c_int, []),
    "mdg_msd_max_lags": (C.c_int, []),
    "mdg_isf_workspace": (C.c_int64, [C.c_int, C.c_int64, C.c_int, C.c_int, C.c_int, C.c_int]),
    "mdg_isf_fwd": (C.c_int, [C.c_int, P, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.POINTER(MdgCell), P, C.c_double, P,
                              C.c_int, P, C.c_int, C.c_int, C.c_int, P, P, P]),
    "mdg_isf_bwd": (C.c_int, [C.c_int, P, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.POINTER(MdgCell), P, C.c_double, P,
                              C.c_int, P, C.c_int, C.c_int, C.c_int, P, P, P, P]),
    "mdg_isf_max_lags": (C.c_int, []),
    "mdg_isf_tile_atoms": (C.c_int, []),
    "mdg_isf_window": (C.c_int, []),
    "mdg_bonded_eval": (C.c_int, [P, C.c_int, C.POINTER(C.c_float), C.c_int, P, C.c_int, C.c_float, C.c_float, P, P, P, P, P, P,
                                  C.c_float, C.c_int, P]),
    "mdg_dihedral_eval": (C.c_int, [P, C.c_int, C.POINTER(C.c_float), P, C.c_int, P, P, C.c_int, P, P, P, P, P, P, P, P,
                                    C.c_float, C.c_int, P]),
    "mdg_dihedral_coeff_grad": (C.c_int, [P, P, P, C.c_int, C.c_int, P, P, P]),
    "mdg_dihedral_phi_fwd": (C.c_int, [P, C.c_int, C.c_int, C.POINTER(C.c_float), P, C.c_int, P, P, P]),
    "mdg_dihedral_phi_bwd": (C.c_int, [P, C.c_int, C.c_int, C.POINTER(C.c_float), P, C.c_int, P, P, P, P, P, P]),
    "mdg_dihedral_hist_scratch": (C.c_int64, [C.c_int64, C.c_int]),
    "mdg_dihedral_hist_fwd": (C.c_int, [P, P, C.c_int64, C.c_int, C.c_float, P, P, P]),
    "mdg_dihedral_hist_bwd": (C.c_int, [P, P, C.c_int64, C.c_int, C.c_float, P, P, P]),
    "mdg_coulomb_partial_size": (C.c_int64, [C.c_int]),
    "mdg_coulomb_eval": (C.c_int, [P, C.c_int, C.POINTER(MdgCell), P, P, P, C.c_int, P, C.POINTER(MdgCoulombConsts), P,
                                   P, P, P, P, P, P, C.c_float, C.c_int, P]),
    "mdg_coulomb_charge_reduce": (C.c_int, [P, P, C.c_int, C.c_int, C.c_int, P, P]),
    "mdg_sw_partial_size": (C.c_int64, [C.c_int]),
    "mdg_sw_eval": (C.c_int, [P, C.c_int, C.POINTER(MdgCell), P, P, P, C.c_int, C.POINTER(MdgSWConsts), P, P,
                              P, P, P, P, P, P, C.c_float, C.c_int, P]),
    "mdg_sw_frames_row_cap": (C.c_int, []),
    "mdg_sw_frames_fwd": (C.c_int, [P, C.c_int, C.c_int, C.POINTER(MdgCell), C.POINTER(MdgSWConsts), P, P, P, P]),
    "mdg_sw_frames_theta_bwd": (C.c_int, [P, P, C.c_int, P, P]),
    "mdg_eam_partial_size": (C.c_int64, [C.c_int]),
    "mdg_eam_eval": (C.c_int, [P, C.c_int, C.POINTER(MdgCell), P, P, P, C.c_int, C.POINTER(MdgEAMConsts), P, P,
                               P, P, P, P, P, P, P, C.c_float, C.c_int, P]),
    "mdg_tersoff_partial_size": (C.c_int64, [C.c_int]),
    "mdg_tersoff_work_size": (C.c_int64, [C.c_int, C.c_int]),
    "mdg_tersoff_eval": (C.c_int, [P, C.c_int, C.POINTER(MdgCell), P, P, P, C.c_int, C.POINTER(MdgTersoffConsts), P, P,
                                   P, P, P, P, P, P, P, C.c_float, C.c_int, P]),
    "mdg_tersoff_multi_partial_size": (C.c_int64, [C.c_int]),
    "mdg_tersoff_multi_work_size": (C.c_int64, [C.c_int, C.c_int]),
    "mdg_tersoff_multi_table_size": (C.c_int64, [C.c_int]),
    "mdg_tersoff_multi_eval": (C.c_int, [P, C.c_int, C.POINTER(MdgCell), P, P, P, C.c_int, P, C.c_int, P, P,
                                         P, P, P, P, P, P, P, C.c_float, C.c_int, P]),
    "mdg_sw_multi_partial_size": (C.c_int64, [C.c_int]),
    "mdg_sw_multi_table_size": (C.c_int64, [C.c_int]),
    "mdg_sw_multi_eval": (C.c_int, [P, C.c_int, C.POINTER(MdgCell), P, P, P, C.c_int, P, C.c_int, P, P,
                                    P, P, P, P, P, P, C.c_float, C.c_int, P]),
    "mdg_eam_table_partial_size": (C.c_int64, [C.c_int]),
    "mdg_eam_table_size": (C.c_int64, [C.c_int, C.c_int, C.c_int]),
    "mdg_eam_table_fx_size": (C.c_int64, [C.c_int, C.c_int, C.c_int]),
    "mdg_eam_table_eval": (C.c_int, [P, C.c_int, C.POINTER(MdgCell), P, P, P, C.c_int, P, C.POINTER(MdgEAMTableConsts), P, P,
                                     P, P, P, P, P, P, P, P, C.c_float, C.c_int, P]),
    "mdg_eam_table_frames_lds_floats": (C.c_int, []),
    "mdg_eam_table_frames_fwd": (C.c_int, [P, C.c_int, C.c_int, C.POINTER(MdgCell), P, C.POINTER(MdgEAMTableConsts), P, C.c_int,
                                           P, P, P]),
    "mdg_eam_table_frames_nodes_bwd": (C.c_int, [P, C.c_int, C.c_int, C.POINTER(MdgCell), P, C.POINTER(MdgEAMTableConsts), P, P,
                                                 P, P, P, P]),
    "mdg_eam_frames_fwd": (C.c_int, [P, C.c_int, C.c_int, C.POINTER(MdgCell), C.POINTER(MdgEAMConsts), P, P, P, P]),
    "mdg_tersoff_frames_row_cap": (C.c_int, []),
    "mdg_tersoff_frames_fwd": (C.c_int, [P, C.c_int, C.c_int, C.POINTER(MdgCell), C.POINTER(MdgTersoffConsts), P, P, P, P]),
    "mdg_tersoff_multi_frames_fwd": (C.c_int, [P, C.c_int, C.c_int, C.POINTER(MdgCell), P, C.c_int, P, P, P, P]),
    "mdg_frames_theta_bwd": (C.c_int, [P, P, C.c_int, C.c_int, P, P]),
    "mdg_ewald_workspace": (C.c_int64, [C.c_int, C.c_int, C.c_int]),
    "mdg_ewald_eval": (C.c_int, [P, C.c_int, C.c_int, C.POINTER(MdgCell), P, P, P, C.c_int, P, P, P, P, P, P, P, C.c_float,
                                 C.c_int, P]),
    "mdg_ewald_excl_partial_size": (C.c_int64, [C.c_int, C.c_int]),
    "mdg_ewald_excl_eval": (C.c_int, [P, C.c_int, C.c_int, C.POINTER(C.c_float), P, P, P, P, C.c_double, C.c_double, P,
                                      P, P, P, P, P, P, C.c_float, C.c_int, P]),
}

EXPORTED_SYMBOLS = tuple(_SIGNATURES)
_lib = None


class MdgradLibraryError(RuntimeError):
    pass


def load():
    """Load (once) and return the ctypes handle.  Raises MdgradLibraryError when the shared
    library has not been built -- there is deliberately no CPU / pure-torch fallback."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise MdgradLibraryError(
            "libmdgrad_hip.so not found at %s -- build it with `python -c 'import __graft_entry__ as g; "
            "g.build()'` (hipcc --offload-arch=gfx950).  mdgrad_amd has no CPU fallback." % LIB_PATH)
    lib = C.CDLL(LIB_PATH)          # torch is imported above: its libamdhip64 is already resident
    for name, (res, args) in _SIGNATURES.items():
        fn = getattr(lib, name)     # AttributeError here = header/library mismatch
        fn.restype, fn.argtypes = res, args
    _lib = lib
    return lib


def check(rc, what):
    if rc != 0:
        msg = load().mdg_last_error()
        raise RuntimeError("%s failed (%d): %s" % (what, rc, msg.decode() if msg else "?"))


def ptr(t):
    """Device pointer of a contiguous tensor (None -> NULL)."""
    if t is None:
        return None
    if not t.is_contiguous():
        raise ValueError("mdgrad_amd: non-contiguous tensor passed to the HIP library")
    return C.c_void_p(t.data_ptr())


def stream_ptr(device=None):
    """The current HIP stream of `device` (torch.device / index / None) as a void*: one call into torch's C layer
    (torch.cuda.current_stream() builds a Stream object per call -- ~5 us, several hundred times per MD pass)."""
    if device is None:
        idx = torch.cuda.current_device()
    elif isinstance(device, int):
        idx = device
    else:
        idx = device.index if isinstance(device, torch.device) else torch.device(device).index
        if idx is None:
            idx = torch.cuda.current_device()
    return C.c_void_p(torch._C._cuda_getCurrentRawStream(idx))


def require_gpu(t, name="tensor", dtype=torch.float32):
    if not t.is_cuda:
        raise RuntimeError("mdgrad_amd: %s must live on a HIP device (got %s); the hot path has no CPU "
                           "implementation" % (name, t.device))
    if dtype is not None and t.dtype != dtype:
        raise TypeError("mdgrad_amd: %s must be %s (got %s)" % (name, dtype, t.dtype))
    return t


def make_cell(cell):
    """MdgCell from a [3] or [3,3] tensor/array (host side).  The inverse is computed with
    torch (fp32, CPU) like the reference's `cell.inverse()` (torchmd/topology.py:59)."""
    c = torch.as_tensor(cell, dtype=torch.float32).detach().cpu()
    if c.dim() == 1:
        c = torch.diag(c)
    inv = c.inverse()
    mc = MdgCell()
    flat, finv = c.reshape(-1).tolist(), inv.reshape(-1).tolist()
    for k in range(9):
        mc.h[k] = flat[k]
        mc.inv[k] = finv[k]
    off = [flat[k] for k in (1, 2, 3, 5, 6, 7)]
    mc.diag = int(all(x == 0.0 for x in off))
    return mc
