"""ctypes binding of libaether_hip.so (include/aether_hip.h).

The library is the product; this module only declares its prototypes.  There is
no CPU fallback: if the shared object is missing or does not load, importing
fails loudly with instructions (build with `python -c "import __graft_entry__ as
g; g.build()"` or `make -C aether_primitives_amd/csrc`).
"""
import ctypes as C
import os

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(_HERE, "lib", "libaether_hip.so")
# tools/ only: AETH_LAB_LIB=1 loads the lab build of the SAME sources (`make -C aether_primitives_amd/csrc LAB=1`),
# which keeps the measured-and-not-kept routes reachable through their AETH_* knobs (csrc/aeth_internal.h, lab_int)
if os.environ.get("AETH_LAB_LIB") == "1":
    LIB_PATH = os.path.join(_HERE, "lib", "libaether_hip_lab.so")

OK = 0
E_LEN, E_ARG, E_ALIGN, E_HIP, E_NOMEM, E_UNSUPPORTED = -1, -2, -3, -4, -5, -6

vp, sz, f32, i32 = C.c_void_p, C.c_size_t, C.c_float, C.c_int
pvp = C.POINTER(C.c_void_p)
psz = C.POINTER(C.c_size_t)
u64 = C.c_uint64


class Cf32(C.Structure):
    """aeth_cf32 by value (aeth_seq_chips)"""
    _fields_ = [("re", C.c_float), ("im", C.c_float)]


class SyncRecord(C.Structure):
    """aeth_sync_record: 48 bytes"""
    _fields_ = [("re", C.c_double), ("im", C.c_double), ("mass", C.c_double), ("n", C.c_uint64), ("n_nonfinite", C.c_uint64),
                ("reserved", C.c_uint64)]


class MovPeak(C.Structure):
    """aeth_mov_peak: 64 bytes"""
    _fields_ = [("index", C.c_uint64), ("first", C.c_uint64), ("p_re", C.c_double), ("p_im", C.c_double), ("r", C.c_double),
                ("r_lag", C.c_double), ("metric", C.c_float), ("n_nan", C.c_uint32), ("reserved", C.c_uint64)]


# name -> (restype, argtypes); mirrors include/aether_hip.h declaration by declaration
PROTOTYPES = {
    "aeth_last_error": (C.c_char_p, []),
    "aeth_version": (i32, []),
    "aeth_device_count": (i32, [C.POINTER(i32)]),
    "aeth_ctx_create": (i32, [i32, pvp]),
    "aeth_ctx_create_on_stream": (i32, [i32, vp, pvp]),
    "aeth_ctx_destroy": (i32, [vp]),
    "aeth_ctx_sync": (i32, [vp]),
    "aeth_ctx_set_overlap": (i32, [vp, i32]),
    "aeth_ctx_overlap": (i32, [vp]),
    "aeth_ctx_lane_counts": (i32, [vp, C.POINTER(u64), C.POINTER(u64)]),
    "aeth_ctx_stream": (vp, [vp]),
    "aeth_ctx_device": (i32, [vp]),
    "aeth_dev_alloc": (i32, [vp, sz, pvp]),
    "aeth_dev_free": (i32, [vp, vp]),
    "aeth_upload": (i32, [vp, vp, vp, sz]),
    "aeth_download": (i32, [vp, vp, vp, sz]),
    "aeth_copy_dev": (i32, [vp, vp, vp, sz]),
    "aeth_event_create": (i32, [vp, pvp]),
    "aeth_event_destroy": (i32, [vp]),
    "aeth_event_record": (i32, [vp]),
    "aeth_event_sync": (i32, [vp]),
    "aeth_event_elapsed_ms": (i32, [vp, vp, C.POINTER(f32)]),
    "aeth_vec_scale": (i32, [vp, vp, sz, f32]),
    "aeth_vec_mul": (i32, [vp, vp, sz, vp, sz]),
    "aeth_vec_div": (i32, [vp, vp, sz, vp, sz]),
    "aeth_vec_conj": (i32, [vp, vp, sz]),
    "aeth_vec_add": (i32, [vp, vp, sz, vp, sz]),
    "aeth_vec_sub": (i32, [vp, vp, sz, vp, sz]),
    "aeth_vec_mirror": (i32, [vp, vp, sz]),
    "aeth_vec_clone": (i32, [vp, vp, sz, vp, sz]),
    "aeth_vec_zero": (i32, [vp, vp, sz]),
    "aeth_vec_mirror_frames": (i32, [vp, vp, sz, sz]),
    "aeth_vec_mul_frames": (i32, [vp, vp, sz, sz, vp, sz]),
    "aeth_host_vec_scale": (i32, [vp, vp, sz, f32]),
    "aeth_host_vec_mul": (i32, [vp, vp, sz, vp, sz]),
    "aeth_host_vec_div": (i32, [vp, vp, sz, vp, sz]),
    "aeth_host_vec_conj": (i32, [vp, vp, sz]),
    "aeth_host_vec_add": (i32, [vp, vp, sz, vp, sz]),
    "aeth_host_vec_sub": (i32, [vp, vp, sz, vp, sz]),
    "aeth_host_vec_mirror": (i32, [vp, vp, sz]),
    "aeth_host_vec_clone": (i32, [vp, vp, sz, vp, sz]),
    "aeth_host_vec_zero": (i32, [vp, vp, sz]),
    "aeth_scale_factor": (f32, [i32, sz, f32]),
    "aeth_scale_apply": (i32, [vp, i32, f32, vp, sz]),
    "aeth_fft_create": (i32, [vp, sz, sz, pvp]),
    "aeth_fft_destroy": (i32, [vp]),
    "aeth_fft_len": (sz, [vp]),
    "aeth_fft_algorithm": (C.c_char_p, [vp]),
    "aeth_fft_route": (C.c_char_p, [vp]),
    "aeth_fft_exec": (i32, [vp, vp, sz, vp, sz, i32, i32, f32]),
    "aeth_fft_exec_mirrored": (i32, [vp, vp, sz, vp, sz, i32, i32, f32]),
    "aeth_fft_exec_interpolate": (i32, [vp, vp, sz, sz, i32, i32, f32, vp, sz, sz, i32, psz]),
    "aeth_fft_exec_host": (i32, [vp, vp, sz, vp, sz, i32, i32, f32]),
    "aeth_fft_exec_tmp_host": (i32, [vp, vp, sz, i32, i32, f32, pvp]),
    "aeth_fft_exec_tmp": (i32, [vp, vp, sz, sz, i32, i32, f32, pvp]),
    "aeth_fft_mul_ifft": (i32, [vp, vp, sz, sz, vp, sz, i32, f32, i32, f32]),
    "aeth_fft_mul_ifft_demod": (i32, [vp, vp, sz, sz, vp, sz, i32, f32, i32, f32, i32, vp, vp, sz, i32]),
    "aeth_fir_create": (i32, [vp, vp, sz, sz, pvp]),
    "aeth_fir_destroy": (i32, [vp]),
    "aeth_fir_ntaps": (sz, [vp]),
    "aeth_fir_fft_len": (sz, [vp]),
    "aeth_fir_hop": (sz, [vp]),
    "aeth_fir_exec": (i32, [vp, vp, vp, sz, vp]),
    "aeth_fir_exec_decim": (i32, [vp, vp, vp, sz, vp, sz]),
    "aeth_fir_exec_host": (i32, [vp, vp, vp, sz, vp]),
    "aeth_pool_create": (i32, [vp, sz, sz, i32, pvp]),
    "aeth_pool_destroy": (i32, [vp]),
    "aeth_pool_take": (i32, [vp, pvp]),
    "aeth_pool_take_or_make": (i32, [vp, pvp]),
    "aeth_pool_give_back": (i32, [vp, vp]),
    "aeth_pool_len": (sz, [vp]),
    "aeth_pool_cap": (sz, [vp]),
    "aeth_pool_elem_bytes": (sz, [vp]),
    "aeth_host_register": (i32, [vp, vp, sz]),
    "aeth_host_unregister": (i32, [vp, vp]),
    "aeth_host_is_pinned": (i32, [vp, sz]),
    "aeth_vec_chain": (i32, [vp, vp, sz, vp, sz]),
    "aeth_vec_fft": (i32, [vp, vp, sz, i32, i32, f32]),
    "aeth_host_vec_fft": (i32, [vp, vp, sz, i32, i32, f32]),
    "aeth_stream_out_count": (sz, [vp, vp, sz]),
    "aeth_stream_host": (i32, [vp, vp, vp, sz, vp, sz, sz, vp]),
    "aeth_stream_chain_out_count": (sz, [vp, vp, sz, sz]),
    "aeth_stream_host_chain": (i32, [vp, vp, sz, vp, sz, vp, sz, sz, vp, vp]),
    "aeth_stream_host_util": (i32, [vp, vp, vp, sz, vp, sz, sz, vp]),
    "aeth_ctx_trim": (i32, [vp]),
    "aeth_test_fail_staging_after": (None, [i32]),
    "aeth_fir_stream_host": (i32, [vp, vp, sz, vp, sz, vp]),
    "aeth_fir_stream_host_util": (i32, [vp, vp, sz, vp, sz, vp]),
    "aeth_fir_stream_file": (i32, [vp, C.c_char_p, C.c_char_p, sz, vp]),
    "aeth_stream_file": (i32, [vp, vp, C.c_char_p, C.c_char_p, sz, vp]),
    "aeth_file_count_structs": (i32, [C.c_char_p, sz, psz]),
    "aeth_file_read": (i32, [C.c_char_p, sz, vp, sz, sz]),
    "aeth_file_write": (i32, [C.c_char_p, vp, sz, sz, i32]),
    "aeth_interpolate": (i32, [vp, vp, sz, vp, sz, sz, i32, psz]),
    "aeth_interpolate_frames": (i32, [vp, vp, sz, sz, vp, sz, sz, i32, psz]),
    "aeth_host_interpolate": (i32, [vp, vp, sz, vp, sz, sz, i32, psz]),
    "aeth_downsample": (i32, [vp, vp, sz, vp, sz, sz]),
    "aeth_host_downsample": (i32, [vp, vp, sz, vp, sz, sz]),
    "aeth_downsample_release": (i32, [vp, vp, sz, vp, sz, sz, i32]),
    "aeth_host_downsample_release": (i32, [vp, vp, sz, vp, sz, sz, i32]),
    "aeth_modulate": (i32, [vp, vp, sz, i32, vp, vp, sz]),
    "aeth_modulate_awgn": (i32, [vp, vp, sz, i32, vp, vp, sz, f32, C.c_uint64, C.c_uint64]),
    "aeth_demod_naive": (i32, [vp, vp, sz, i32, vp, vp, sz, i32]),
    "aeth_demod_soft": (i32, [vp, vp, sz, i32, vp, f32, vp, sz]),
    "aeth_awgn_apply": (i32, [vp, vp, sz, f32, C.c_uint64, C.c_uint64]),
    "aeth_awgn_fill": (i32, [vp, vp, sz, f32, C.c_uint64, C.c_uint64]),
    "aeth_rng_philox4x32_10": (i32, [vp, vp, sz, vp]),
    "aeth_rng_philox4x32": (i32, [vp, vp, sz, i32, vp]),
    "aeth_rng_normal_pairs": (i32, [vp, vp, sz, vp]),
    "aeth_vec_stats": (i32, [vp, vp, sz, vp]),
    "aeth_host_vec_stats": (i32, [vp, vp, sz, vp]),
    "aeth_vec_levels": (i32, [vp, vp, sz, i32, vp, sz]),
    "aeth_fft_exec_levels": (i32, [vp, vp, sz, sz, i32, i32, f32, i32, i32, vp, sz]),
    "aeth_corr_create": (i32, [vp, vp, sz, sz, pvp]),
    "aeth_corr_destroy": (i32, [vp]),
    "aeth_corr_nref": (sz, [vp]),
    "aeth_corr_fft_len": (sz, [vp]),
    "aeth_corr_hop": (sz, [vp]),
    "aeth_corr_exec": (i32, [vp, vp, vp, sz, vp]),
    "aeth_corr_exec_levels": (i32, [vp, vp, vp, sz, i32, vp, sz]),
    "aeth_corr_search": (i32, [vp, vp, vp, sz, vp, sz, vp]),
    "aeth_seq_window": (i32, [vp, u64, u64, C.POINTER(u64)]),
    "aeth_seq_create": (i32, [vp, vp, sz, pvp]),
    "aeth_seq_destroy": (i32, [vp]),
    "aeth_seq_nregs": (sz, [vp]),
    "aeth_seq_order": (sz, [vp, sz]),
    "aeth_seq_chunk": (sz, [vp]),
    "aeth_seq_bits": (i32, [vp, vp, u64, vp, sz]),
    "aeth_seq_scramble": (i32, [vp, vp, u64, vp, vp, sz]),
    "aeth_seq_chips": (i32, [vp, vp, u64, Cf32, Cf32, vp, sz]),
    "aeth_seq_spread": (i32, [vp, vp, u64, vp, sz, sz, vp, sz]),
    "aeth_host_seq_bits": (i32, [vp, vp, u64, vp, sz]),
    "aeth_chan_create": (i32, [vp, vp, sz, sz, sz, i32, sz, pvp]),
    "aeth_chan_destroy": (i32, [vp]),
    "aeth_chan_channels": (sz, [vp]),
    "aeth_chan_ntaps": (sz, [vp]),
    "aeth_chan_hop": (sz, [vp]),
    "aeth_chan_phase": (i32, [vp]),
    "aeth_chan_route": (C.c_char_p, [vp]),
    "aeth_chan_tile": (sz, [vp]),
    "aeth_chan_fold": (i32, [vp, vp, vp, sz, u64, vp, sz]),
    "aeth_chan_exec": (i32, [vp, vp, vp, sz, u64, i32, i32, f32, vp, sz]),
    "aeth_chan_exec_levels": (i32, [vp, vp, vp, sz, u64, i32, i32, f32, i32, i32, vp, sz]),
    "aeth_chan_prototype": (i32, [i32, sz, sz, vp]),
    "aeth_vec_frame_sums": (i32, [vp, vp, sz, sz, sz, sz, vp, vp, sz]),
    "aeth_chan_exec_sums": (i32, [vp, vp, vp, sz, u64, i32, i32, f32, i32, sz, i32, vp, vp, sz]),
    "aeth_chan_sums_chunk": (sz, [vp]),
    "aeth_chan_sums_fused": (i32, [vp]),
    "aeth_vec_sum_levels": (i32, [vp, vp, sz, C.c_double, i32, vp]),
    "aeth_synth_create": (i32, [vp, vp, sz, sz, sz, i32, sz, pvp]),
    "aeth_synth_destroy": (i32, [vp]),
    "aeth_synth_channels": (sz, [vp]),
    "aeth_synth_ntaps": (sz, [vp]),
    "aeth_synth_hop": (sz, [vp]),
    "aeth_synth_phase": (i32, [vp]),
    "aeth_synth_route": (C.c_char_p, [vp]),
    "aeth_synth_tile": (sz, [vp]),
    "aeth_synth_history": (sz, [vp]),
    "aeth_synth_unfold": (i32, [vp, vp, vp, sz, u64, vp, sz]),
    "aeth_synth_exec": (i32, [vp, vp, vp, sz, u64, i32, i32, f32, vp, sz]),
    "aeth_synth_dual_window": (i32, [vp, sz, sz, vp]),
    "aeth_resamp_create": (i32, [vp, vp, sz, sz, sz, pvp]),
    "aeth_resamp_destroy": (i32, [vp]),
    "aeth_resamp_up": (sz, [vp]),
    "aeth_resamp_down": (sz, [vp]),
    "aeth_resamp_ntaps": (sz, [vp]),
    "aeth_resamp_history": (sz, [vp]),
    "aeth_resamp_tile": (sz, [vp]),
    "aeth_resamp_route": (C.c_char_p, [vp]),
    "aeth_resamp_out_count": (sz, [vp, sz]),
    "aeth_resamp_exec": (i32, [vp, vp, vp, sz, vp, sz]),
    "aeth_resamp_prototype": (i32, [sz, sz, sz, vp]),
    "aeth_arb_advance": (i32, [u64, u64, sz, vp, vp]),
    "aeth_arb_create": (i32, [vp, vp, sz, sz, pvp]),
    "aeth_arb_destroy": (i32, [vp]),
    "aeth_arb_phases": (sz, [vp]),
    "aeth_arb_ntaps": (sz, [vp]),
    "aeth_arb_history": (sz, [vp]),
    "aeth_arb_tile": (sz, [vp, u64]),
    "aeth_arb_route": (C.c_char_p, [vp, u64]),
    "aeth_arb_exec": (i32, [vp, vp, vp, sz, u64, u64, vp, sz]),
    "aeth_nco_word": (u64, [C.c_double]),
    "aeth_nco_word_at": (u64, [vp, u64]),
    "aeth_nco_phasor": (i32, [u64, vp]),
    "aeth_nco_mix": (i32, [vp, vp, u64, vp, vp, sz]),
    "aeth_nco_tone": (i32, [vp, vp, u64, f32, vp, sz]),
    "aeth_sync_chunk": (sz, []),
    "aeth_sync_line": (i32, [vp, i32, vp, u64, vp, sz, sz, vp, vp]),
    "aeth_sync_lag": (i32, [vp, i32, sz, vp, vp, sz, sz, vp, vp]),
    "aeth_sync_turns": (C.c_double, [vp]),
    "aeth_sync_freq_step": (u64, [vp, i32, sz]),
    "aeth_sync_timing_phase": (u64, [vp, C.c_double]),
    "aeth_mov_history": (sz, [i32, sz, sz]),
    "aeth_mov_grid": (sz, [i32, sz]),
    "aeth_mov_freq_step": (u64, [vp, sz]),
    "aeth_mov_exec": (i32, [vp, i32, sz, sz, vp, vp, sz, vp, vp, vp]),
    "aeth_mov_search": (i32, [vp, i32, sz, sz, C.c_double, C.c_double, vp, vp, sz, sz, vp, vp]),
    "aeth_ofdm_create": (i32, [vp, sz, sz, vp, sz, sz, i32, pvp]),
    "aeth_ofdm_destroy": (i32, [vp]),
    "aeth_ofdm_len": (sz, [vp]),
    "aeth_ofdm_cp": (sz, [vp]),
    "aeth_ofdm_symbol": (sz, [vp]),
    "aeth_ofdm_carriers": (sz, [vp]),
    "aeth_ofdm_route": (C.c_char_p, [vp]),
    "aeth_ofdm_span": (sz, [vp, sz]),
    "aeth_ofdm_demod": (i32, [vp, vp, sz, sz, vp, i32, f32, vp, sz]),
    "aeth_ofdm_mod": (i32, [vp, vp, sz, sz, i32, f32, vp, sz]),
    "aeth_ofdm_estimate": (i32, [vp, vp, vp, sz, sz, f32, i32, vp, vp, vp]),
    "aeth_cc_create": (i32, [vp, vp, sz, sz, sz, pvp]),
    "aeth_cc_destroy": (i32, [vp]),
    "aeth_cc_k": (sz, [vp]),
    "aeth_cc_n": (sz, [vp]),
    "aeth_cc_block": (sz, [vp]),
    "aeth_cc_warmup": (sz, [vp]),
    "aeth_cc_traceback": (sz, [vp]),
    "aeth_cc_history": (sz, [vp]),
    "aeth_cc_encode": (i32, [vp, vp, vp, sz, vp, sz]),
    "aeth_cc_decode": (i32, [vp, vp, vp, sz, vp, sz]),
    "aeth_remap_create": (i32, [vp, vp, sz, sz, pvp]),
    "aeth_remap_destroy": (i32, [vp]),
    "aeth_remap_in_period": (sz, [vp]),
    "aeth_remap_out_period": (sz, [vp]),
    "aeth_remap_in_count": (sz, [vp, sz]),
    "aeth_remap_route": (i32, [vp]),
    "aeth_remap_tile": (sz, [vp]),
    "aeth_remap_exec": (i32, [vp, vp, sz, vp, sz, C.c_uint8]),
    "aeth_remap_puncture": (i32, [vp, sz, vp, sz, psz]),
    "aeth_remap_invert": (i32, [vp, sz, sz, vp]),
    "aeth_remap_compose": (i32, [vp, sz, sz, vp, sz, sz, vp, sz, psz, psz]),
    "aeth_remap_rows_cols": (i32, [sz, sz, vp]),
    "aeth_remap_bicm16": (i32, [sz, sz, vp]),
    "aeth_crc_create": (i32, [vp, C.c_uint32, u64, u64, u64, pvp]),
    "aeth_crc_destroy": (i32, [vp]),
    "aeth_crc_width": (C.c_uint32, [vp]),
    "aeth_crc_poly": (u64, [vp]),
    "aeth_crc_init": (u64, [vp]),
    "aeth_crc_xorout": (u64, [vp]),
    "aeth_crc_residue": (u64, [vp]),
    "aeth_crc_route": (i32, [vp, sz, sz]),
    "aeth_crc_route_frame_bits": (sz, [vp]),
    "aeth_crc_frames_per_workgroup": (sz, [vp, sz]),
    "aeth_crc_named": (i32, [C.c_char_p, C.POINTER(C.c_uint32), C.POINTER(u64), C.POINTER(u64), C.POINTER(u64)]),
    "aeth_crc_host": (i32, [C.c_uint32, u64, u64, u64, vp, sz, C.POINTER(u64)]),
    "aeth_crc_exec": (i32, [vp, vp, sz, sz, vp, vp]),
    "aeth_crc_attach": (i32, [vp, vp, sz, sz, vp]),
    "aeth_crc_check": (i32, [vp, vp, sz, sz, u64, vp, vp, vp]),
    "aeth_bits_pack": (i32, [vp, vp, sz, i32, vp, sz]),
    "aeth_bits_unpack": (i32, [vp, vp, sz, i32, vp, sz]),
    "aeth_ldpc_generator": (i32, [vp, vp, sz]),
    "aeth_ldpc_create": (i32, [vp, vp, pvp]),
    "aeth_ldpc_destroy": (i32, [vp]),
    "aeth_ldpc_n": (sz, [vp]),
    "aeth_ldpc_k": (sz, [vp]),
    "aeth_ldpc_rows": (C.c_uint32, [vp]),
    "aeth_ldpc_cols": (C.c_uint32, [vp]),
    "aeth_ldpc_z": (C.c_uint32, [vp]),
    "aeth_ldpc_edges": (sz, [vp]),
    "aeth_ldpc_lds_bytes": (sz, [vp]),
    "aeth_ldpc_group": (C.c_uint32, [vp]),
    "aeth_ldpc_encode": (i32, [vp, vp, sz, vp, sz]),
    "aeth_ldpc_decode": (i32, [vp, vp, sz, C.c_uint32, C.c_uint32, vp, sz, vp]),
    "aeth_rs_named": (i32, [C.c_char_p, vp]),
    "aeth_rs_generator": (i32, [vp, vp, sz]),
    "aeth_rs_host_encode": (i32, [vp, vp, sz, C.c_uint32, vp, sz]),
    "aeth_rs_host_decode": (i32, [vp, vp, sz, vp, C.c_uint32, C.c_uint32, vp, sz, vp, vp]),
    "aeth_rs_create": (i32, [vp, vp, pvp]),
    "aeth_rs_destroy": (i32, [vp]),
    "aeth_rs_n": (sz, [vp]),
    "aeth_rs_k": (sz, [vp]),
    "aeth_rs_nroots": (C.c_uint32, [vp]),
    "aeth_rs_m": (C.c_uint32, [vp]),
    "aeth_rs_group": (C.c_uint32, [vp]),
    "aeth_rs_lds_bytes": (sz, [vp, C.c_uint32]),
    "aeth_rs_encode": (i32, [vp, vp, sz, C.c_uint32, vp, sz]),
    "aeth_rs_decode": (i32, [vp, vp, sz, vp, C.c_uint32, C.c_uint32, vp, sz, vp, vp]),
    "aeth_polar_rank": (i32, [C.c_uint32, vp, sz]),
    "aeth_polar_mask": (i32, [C.c_uint32, C.c_uint32, vp, sz]),
    "aeth_polar_create": (i32, [vp, C.c_uint32, vp, pvp]),
    "aeth_polar_destroy": (i32, [vp]),
    "aeth_polar_n": (sz, [vp]),
    "aeth_polar_k": (sz, [vp]),
    "aeth_polar_lanes": (C.c_uint32, [vp]),
    "aeth_polar_group": (C.c_uint32, [vp]),
    "aeth_polar_lds_bytes": (sz, [vp]),
    "aeth_polar_encode": (i32, [vp, vp, sz, vp, sz]),
    "aeth_polar_decode": (i32, [vp, vp, sz, vp, C.c_uint32, vp, sz, vp]),
    "aeth_polar_list_create": (i32, [vp, C.c_uint32, vp, C.c_uint32, pvp]),
    "aeth_polar_list_destroy": (i32, [vp]),
    "aeth_polar_list_n": (sz, [vp]),
    "aeth_polar_list_k": (sz, [vp]),
    "aeth_polar_list_paths": (C.c_uint32, [vp]),
    "aeth_polar_list_lanes": (C.c_uint32, [vp]),
    "aeth_polar_list_group": (C.c_uint32, [vp]),
    "aeth_polar_list_lds_bytes": (sz, [vp]),
    "aeth_polar_list_decode": (i32, [vp, vp, sz, C.c_uint32, vp, sz, vp]),
    "aeth_polar_list_pick": (i32, [vp, vp, sz, sz, C.c_uint32, vp, vp, vp]),
    "aeth_turbo_named": (i32, [C.c_char_p, vp]),
    "aeth_turbo_qpp": (i32, [C.c_uint32, C.c_uint32, C.c_uint32, vp, sz]),
    "aeth_turbo_create": (i32, [vp, vp, C.c_uint32, vp, C.c_uint32, C.c_uint32, pvp]),
    "aeth_turbo_destroy": (i32, [vp]),
    "aeth_turbo_k": (sz, [vp]),
    "aeth_turbo_n": (sz, [vp]),
    "aeth_turbo_states": (C.c_uint32, [vp]),
    "aeth_turbo_window": (C.c_uint32, [vp]),
    "aeth_turbo_warmup": (C.c_uint32, [vp]),
    "aeth_turbo_windows": (C.c_uint32, [vp]),
    "aeth_turbo_group": (C.c_uint32, [vp]),
    "aeth_turbo_lds_bytes": (sz, [vp]),
    "aeth_turbo_encode": (i32, [vp, vp, sz, vp, sz]),
    "aeth_turbo_decode": (i32, [vp, vp, sz, C.c_uint32, C.c_uint32, vp, sz, vp]),
}

_lib = None


class AetherError(RuntimeError):
    def __init__(self, code, message):
        super().__init__(f"[{code}] {message}")
        self.code = code
        self.message = message


class LengthMismatch(AetherError, AssertionError):
    """AETH_E_LEN: the reference panics (assert_eq!) with this message."""


def load():
    """Load libaether_hip.so; never falls back to anything else."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise ImportError(
            f"{LIB_PATH} is missing: the HIP backend is not built. Run "
            "`python -c 'import __graft_entry__ as g; g.build()'` (or `make -C aether_primitives_amd/csrc`). "
            "There is no CPU fallback.")
    lib = C.CDLL(LIB_PATH)
    for name, (res, args) in PROTOTYPES.items():
        fn = getattr(lib, name)      # AttributeError if the .so does not export a declared symbol
        fn.restype = res
        fn.argtypes = args
    _lib = lib
    return lib


def check(rc):
    if rc == OK:
        return
    msg = load().aeth_last_error().decode("utf-8", "replace")
    if rc == E_LEN:
        raise LengthMismatch(rc, msg)
    raise AetherError(rc, msg)
