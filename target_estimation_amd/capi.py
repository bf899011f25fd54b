"""ctypes binding of libtarget_estimation_amd.so (the C ABI in include/target_estimation_amd/).

There is no fallback: if the HIP library has not been built, importing the handle raises.
"""
import ctypes as C
import os

from ._build import LIB

_lib = None

c_uint_p = C.POINTER(C.c_uint)
c_double_p = C.POINTER(C.c_double)
c_ubyte_p = C.POINTER(C.c_ubyte)

# every symbol include/target_estimation_amd/*.h declares: name -> (restype, argtypes)
class BatchSequence(C.Structure):
    """target_batch_sequence_c of target_batch_c.h"""
    _fields_ = [("meas_dev", C.c_void_p), ("tick_stride", C.c_long), ("ld", C.c_long),
                ("has_meas_dev", C.c_void_p), ("has_stride", C.c_long),
                ("delta_dev", C.c_void_p), ("pose_dev", C.c_void_p), ("ring_ticks", C.c_long)]


class PoseStream(C.Structure):
    """target_pose_stream_c of target_batch_c.h: the per-tick pose stream of a launched tick"""
    _fields_ = [("pose_dev", C.c_void_p), ("ld", C.c_long), ("tick_stride", C.c_long), ("ring_ticks", C.c_long)]


class InnovStream(C.Structure):
    """target_innov_stream_c of target_batch_c.h: the per-tick innovation / NIS stream of a launched tick"""
    _fields_ = [("nis_dev", C.c_void_p), ("innov_dev", C.c_void_p), ("ld", C.c_long), ("nis_tick_stride", C.c_long),
                ("innov_tick_stride", C.c_long), ("ring_ticks", C.c_long)]


class Reacquire(C.Structure):
    """target_reacquire_c of target_batch_c.h: the re-acquisition policy of a gated call (max_rejects = -1 in a per-batch array:
    no policy for that batch)"""
    _fields_ = [("max_rejects", C.c_int), ("event_dev", C.c_void_p), ("ld", C.c_long), ("tick_stride", C.c_long), ("ring_ticks", C.c_long)]


class StreamSpec(C.Structure):
    """target_stream_c of target_batch_c.h"""
    _fields_ = [("model", C.c_int), ("seed", C.c_ulonglong), ("first_target", C.c_long), ("dt", C.c_double),
                ("availability", C.c_double), ("rpy_noise", C.c_double)]


class AssocOut(C.Structure):
    """target_assoc_out_c of target_batch_c.h: what one batch's slots get from a manager-level association"""
    _fields_ = [("meas_out_dev", C.c_void_p), ("ld", C.c_long), ("has_meas_out_dev", C.c_void_p), ("det_of_slot_dev", C.c_void_p),
                ("d2_of_slot_dev", C.c_void_p)]


class DupOut(C.Structure):
    """target_dup_out_c of target_batch_c.h: what one batch's slots get from a duplicate search"""
    _fields_ = [("dup_out_dev", C.c_void_p), ("partner_batch_dev", C.c_void_p), ("partner_slot_dev", C.c_void_p), ("d2_of_slot_dev", C.c_void_p)]


class Lifecycle(C.Structure):
    """target_lifecycle_c of target_batch_c.h: the policy of a track-lifecycle call"""
    _fields_ = [("max_misses", C.c_int), ("birth_type", C.c_int), ("first_id", C.c_uint), ("max_births", C.c_long), ("dt0", C.c_double),
                ("t_birth", C.c_double), ("Q", c_double_p), ("R", c_double_p), ("P0", c_double_p)]


SIGNATURES = {
    # target_manager_c.h (the reference's ten symbols)
    "target_manager_new": (C.c_void_p, [C.c_char_p]),
    "target_manager_init": (None, [C.c_void_p, C.c_uint, C.c_double, c_double_p, C.c_double]),
    "target_manager_update_meas": (None, [C.c_void_p, C.c_uint, C.c_double, c_double_p]),
    "target_manager_update": (None, [C.c_void_p, C.c_uint, C.c_double]),
    "target_manager_get_est_pose": (C.c_bool, [C.c_void_p, C.c_uint, c_double_p]),
    "target_manager_get_est_twist": (C.c_bool, [C.c_void_p, C.c_uint, c_double_p]),
    "target_manager_get_est_acceleration": (C.c_bool, [C.c_void_p, C.c_uint, c_double_p]),
    "target_manager_get_n_measurements": (C.c_int, [C.c_void_p, C.c_uint]),
    "target_manager_log": (None, [C.c_void_p]),
    "target_manager_delete": (None, [C.c_void_p]),
    # target_batch_c.h
    "target_manager_new_ex": (C.c_void_p, [C.c_char_p, C.c_int, C.c_int]),
    "target_manager_set_stream": (C.c_int, [C.c_void_p, C.c_void_p]),
    "target_manager_synchronize": (C.c_int, [C.c_void_p]),
    "target_manager_set_log_directory": (C.c_int, [C.c_void_p, C.c_char_p]),
    "target_manager_last_error": (C.c_char_p, []),
    "target_intersection_solver_new": (C.c_void_p, [C.c_void_p, C.c_uint]),
    "target_intersection_solver_delete": (None, [C.c_void_p]),
    "target_intersection_solver_get_time_with_sphere": (C.c_double, [C.c_void_p, C.c_uint, C.c_double, c_double_p, C.c_double]),
    "target_intersection_solver_get_pose_with_sphere": (C.c_bool, [C.c_void_p, C.c_uint, C.c_double, C.c_double, C.c_double, c_double_p,
                                                                   C.c_double, c_double_p]),
    "target_intersection_solver_last_errors": (None, [C.c_void_p, c_double_p, c_double_p]),
    "target_manager_set_log_targets": (C.c_int, [C.c_void_p, c_uint_p, C.c_long]),
    "target_manager_set_keep_measurement": (C.c_int, [C.c_void_p, C.c_int]),
    "target_manager_get_measured_pose": (C.c_bool, [C.c_void_p, C.c_uint, c_double_p]),
    "target_manager_get_period_estimate": (C.c_bool, [C.c_void_p, C.c_uint, c_double_p]),
    "target_manager_get_estimated_transform": (C.c_bool, [C.c_void_p, C.c_uint, c_double_p]),
    "target_manager_get_n": (C.c_int, [C.c_void_p, C.c_uint]),
    "target_manager_get_m": (C.c_int, [C.c_void_p, C.c_uint]),
    "target_manager_get_model_matrices": (C.c_bool, [C.c_void_p, C.c_uint, c_double_p, c_double_p, c_double_p]),
    "target_manager_init_typed": (C.c_int, [C.c_void_p, C.c_int, C.c_uint, C.c_double, C.c_double, c_double_p,
                                            c_double_p, c_double_p, c_double_p, c_double_p, c_double_p]),
    "target_manager_init_batch": (C.c_long, [C.c_void_p, c_uint_p, C.c_long, C.c_double, C.c_double, c_double_p,
                                             c_double_p, c_double_p]),
    "target_manager_init_batch_typed": (C.c_long, [C.c_void_p, C.c_int, c_uint_p, C.c_long, C.c_double, C.c_double,
                                                   c_double_p, c_double_p, c_double_p, C.c_int, c_double_p,
                                                   c_double_p, c_double_p]),
    "target_manager_init_batch_classes": (C.c_long, [C.c_void_p, C.c_int, c_uint_p, C.c_long, C.c_double, C.c_double, C.c_long,
                                                     c_double_p, c_double_p, c_double_p, c_uint_p, c_double_p, c_double_p, c_double_p]),
    "target_batch_num_classes": (C.c_int, [C.c_void_p]),
    "target_manager_erase": (C.c_int, [C.c_void_p, C.c_uint]),
    "target_manager_erase_batch": (C.c_long, [C.c_void_p, C.POINTER(C.c_uint), C.c_long]),
    "target_manager_size": (C.c_long, [C.c_void_p]),
    "target_manager_get_available_targets": (C.c_long, [C.c_void_p, c_uint_p, C.c_long]),
    "target_manager_update_meas_batch": (C.c_long, [C.c_void_p, c_uint_p, C.c_long, C.c_double, c_double_p, c_ubyte_p]),
    "target_manager_update_all": (C.c_int, [C.c_void_p, C.c_double]),
    "target_manager_get_est_batch": (C.c_long, [C.c_void_p, c_uint_p, C.c_long, c_double_p, c_double_p, c_double_p, c_ubyte_p]),
    "target_manager_get_est_at_batch": (C.c_long, [C.c_void_p, c_uint_p, C.c_long, C.c_double, c_double_p, c_double_p,
                                                   c_double_p, c_ubyte_p]),
    "target_manager_get_state_batch": (C.c_long, [C.c_void_p, c_uint_p, C.c_long, c_double_p, c_double_p]),
    "target_manager_get_time": (C.c_int, [C.c_void_p, C.c_uint, c_double_p]),
    "target_manager_get_intersection_time_with_sphere": (C.c_double, [C.c_void_p, C.c_uint, C.c_double, c_double_p, C.c_double]),
    "target_manager_get_intersection_pose_with_sphere": (C.c_bool, [C.c_void_p, C.c_uint, C.c_double, c_double_p, C.c_double,
                                                                    c_double_p, c_double_p]),
    "target_manager_intersect_sphere_batch": (C.c_long, [C.c_void_p, c_uint_p, C.c_long, C.c_double, c_double_p, C.c_double,
                                                         c_double_p, c_double_p, c_ubyte_p]),
    "target_manager_intersect_sphere_converged_batch": (C.c_long, [C.c_void_p, c_uint_p, C.c_long, C.c_double, C.c_double, C.c_double,
                                                                   c_double_p, C.c_double, C.c_int, c_double_p, c_double_p,
                                                                   c_ubyte_p, c_ubyte_p, c_double_p]),
    "target_batch_intersect_sphere_converged_dev": (C.c_int, [C.c_void_p, C.c_double, C.c_double, C.c_double, c_double_p, C.c_double,
                                                              C.c_int, C.c_void_p, C.c_void_p, C.c_void_p]),
    "target_batch_gate_update_dev": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_double, C.c_double, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p]),
    # the k soonest crossings: device pointers as void*, host arrays typed
    "target_batch_select_soonest_dev": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_double, C.c_double, C.c_long,
                                                  C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
    "target_batch_select_soonest": (C.c_long, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_double, C.c_double, C.c_long,
                                               c_uint_p, C.POINTER(C.c_int), c_double_p, c_double_p]),
    "target_manager_select_soonest": (C.c_long, [C.c_void_p, C.c_void_p, C.c_long, C.POINTER(C.c_void_p), C.c_double, C.c_double, C.c_long,
                                                 c_uint_p, C.POINTER(C.c_int), C.POINTER(C.c_int), c_double_p, c_double_p]),
    "target_manager_select_soonest_dev": (C.c_int, [C.c_void_p, C.c_void_p, C.c_long, C.POINTER(C.c_void_p), C.c_double, C.c_double,
                                                    C.c_long, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
    # covariance and time spread at a crossing: origin a host double[3], device pointers as void*, host arrays typed
    "target_batch_crossing_cov_dev": (C.c_int, [C.c_void_p, C.c_double, c_double_p, C.c_double, C.c_void_p, C.c_void_p, C.c_long, C.c_double,
                                                C.c_double, C.c_void_p, C.c_void_p, C.c_void_p]),
    "target_manager_crossing_cov_dev": (C.c_int, [C.c_void_p, C.c_double, c_double_p, C.c_double, C.c_void_p, C.c_void_p, C.c_void_p, C.c_long,
                                                  C.c_double, C.c_double, C.c_void_p, C.c_void_p, C.c_void_p]),
    "target_manager_crossing_cov_batch": (C.c_long, [C.c_void_p, c_uint_p, C.c_long, C.c_double, c_double_p, C.c_double, c_double_p, C.c_double,
                                                     C.c_double, c_double_p, c_double_p, c_ubyte_p]),
    # association of unlabelled detections: device pointers as void*, host arrays typed
    "target_batch_associate_dev": (C.c_int, [C.c_void_p, C.c_double, C.c_void_p, C.c_long, C.c_double, C.c_int, C.c_void_p, C.c_long, C.c_void_p,
                                             C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
    "target_batch_associate": (C.c_long, [C.c_void_p, C.c_double, c_double_p, C.c_long, C.c_double, C.c_int, C.c_void_p, C.c_long, C.c_void_p,
                                          c_uint_p, C.POINTER(C.c_int), c_double_p, C.POINTER(C.c_long), C.POINTER(C.c_long),
                                          C.POINTER(C.c_int)]),
    "target_manager_associate_dev": (C.c_int, [C.c_void_p, C.c_double, C.c_void_p, C.c_long, C.c_double, C.c_int, C.POINTER(AssocOut), C.c_long,
                                               C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
    "target_manager_associate": (C.c_long, [C.c_void_p, C.c_double, c_double_p, C.c_long, C.c_double, C.c_int, C.POINTER(AssocOut), C.c_long,
                                            c_uint_p, C.POINTER(C.c_int), C.POINTER(C.c_int), c_double_p, C.POINTER(C.c_long),
                                            C.POINTER(C.c_long), C.POINTER(C.c_int)]),
    # ... and its grid form: the same lists with `double cell` after rounds
    "target_batch_associate_grid_dev": (C.c_int, [C.c_void_p, C.c_double, C.c_void_p, C.c_long, C.c_double, C.c_int, C.c_double, C.c_void_p,
                                                  C.c_long, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
    "target_batch_associate_grid": (C.c_long, [C.c_void_p, C.c_double, c_double_p, C.c_long, C.c_double, C.c_int, C.c_double, C.c_void_p,
                                               C.c_long, C.c_void_p, c_uint_p, C.POINTER(C.c_int), c_double_p, C.POINTER(C.c_long),
                                               C.POINTER(C.c_long), C.POINTER(C.c_int)]),
    "target_manager_associate_grid_dev": (C.c_int, [C.c_void_p, C.c_double, C.c_void_p, C.c_long, C.c_double, C.c_int, C.c_double,
                                                    C.POINTER(AssocOut), C.c_long, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
    "target_manager_associate_grid": (C.c_long, [C.c_void_p, C.c_double, c_double_p, C.c_long, C.c_double, C.c_int, C.c_double,
                                                 C.POINTER(AssocOut), C.c_long, c_uint_p, C.POINTER(C.c_int), C.POINTER(C.c_int), c_double_p,
                                                 C.POINTER(C.c_long), C.POINTER(C.c_long), C.POINTER(C.c_int)]),
    # track lifecycle: device pointers as void* (the masks: an array of them), host arrays typed
    "target_manager_lifecycle": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_long, C.POINTER(C.c_void_p), C.c_long, C.POINTER(Lifecycle),
                                           c_uint_p, C.c_long, C.POINTER(C.c_long)]),
    # duplicate tracks: device pointers as void*, host arrays typed
    "target_manager_find_duplicates_dev": (C.c_int, [C.c_void_p, C.c_double, C.c_double, C.c_int, C.c_double, C.c_int, C.POINTER(DupOut), C.c_long,
                                                     C.c_void_p]),
    "target_manager_retire_duplicates": (C.c_int, [C.c_void_p, C.c_double, C.c_double, C.c_int, C.c_double, C.c_int, c_uint_p, c_uint_p, C.c_long,
                                                   C.POINTER(C.c_long)]),
    "target_batch_track_counts": (C.c_int, [C.c_void_p, c_ubyte_p, c_ubyte_p]),
    "target_manager_get_track_counts": (C.c_int, [C.c_void_p, C.c_uint, C.POINTER(C.c_int), C.POINTER(C.c_int)]),
    "target_batch_intersect_sphere_dev": (C.c_int, [C.c_void_p, C.c_double, c_double_p, C.c_double, C.c_void_p, C.c_void_p]),
    "target_comm_unique_id": (C.c_int, [C.c_char_p]),
    "target_comm_new": (C.c_void_p, [C.c_char_p, C.c_int, C.c_int]),
    "target_comm_delete": (None, [C.c_void_p]),
    "target_manager_gather_pose_begin": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.POINTER(C.c_long), C.c_void_p]),
    "target_manager_gather_pose_wait": (C.c_int, [C.c_void_p, C.POINTER(C.c_float)]),
    "target_manager_gather_pose_wait_for": (C.c_int, [C.c_void_p, C.c_double, C.POINTER(C.c_float)]),
    "target_ingest_new": (C.c_void_p, [C.c_void_p, C.c_int, c_double_p, c_double_p, c_double_p]),
    "target_ingest_delete": (None, [C.c_void_p]),
    "target_ingest_set_expiration_time": (None, [C.c_void_p, C.c_double]),
    "target_ingest_set_token_name": (None, [C.c_void_p, C.c_char_p]),
    "target_ingest_push": (C.c_int, [C.c_void_p, C.c_uint, C.c_double, c_double_p]),
    "target_ingest_push_named": (C.c_int, [C.c_void_p, C.c_char_p, C.c_double, c_double_p]),
    "target_ingest_tick": (C.c_long, [C.c_void_p, C.c_double, C.c_double, c_uint_p, c_double_p, C.c_long]),
    "target_manager_num_batches": (C.c_int, [C.c_void_p]),
    "target_manager_get_batch": (C.c_void_p, [C.c_void_p, C.c_int]),
    "target_manager_get_batch_of_type": (C.c_void_p, [C.c_void_p, C.c_int]),
    "target_batch_size": (C.c_long, [C.c_void_p]),
    "target_batch_type": (C.c_int, [C.c_void_p]),
    "target_batch_dtype": (C.c_int, [C.c_void_p]),
    "target_batch_state_dim": (C.c_int, [C.c_void_p]),
    "target_batch_meas_dim": (C.c_int, [C.c_void_p]),
    "target_batch_lanes_per_target": (C.c_int, [C.c_void_p]),
    "target_batch_is_symmetric_packed": (C.c_int, [C.c_void_p]),
    "target_batch_layout": (C.c_int, [C.c_void_p]),
    "target_batch_shared_axes": (C.c_int, [C.c_void_p]),
    "target_manager_set_shared_axes": (C.c_int, [C.c_void_p, C.c_int]),
    "target_batch_uniform_tiles": (C.c_long, [C.c_void_p]),
    "target_manager_set_uniform_tiles": (C.c_int, [C.c_void_p, C.c_int]),
    "target_batch_record_words": (C.c_int, [C.c_void_p]),
    "target_batch_algorithmic_bytes": (C.c_long, [C.c_void_p]),
    "target_batch_resident_bytes_per_target": (C.c_double, [C.c_void_p]),
    "target_batch_slot_ids": (C.c_long, [C.c_void_p, c_uint_p, C.c_long]),
    "target_batch_step": (C.c_int, [C.c_void_p, C.c_double, C.c_void_p, C.c_long, C.c_void_p]),
    "target_batch_step_host": (C.c_int, [C.c_void_p, C.c_double, C.c_void_p, C.c_long, C.c_void_p]),
    "target_batch_step_sequence": (C.c_int, [C.c_void_p, C.c_long, C.c_double, C.c_void_p, C.c_long, C.c_long, C.c_void_p, C.c_long, C.c_int]),
    "target_batch_step_sequence_ring": (C.c_int, [C.c_void_p, C.c_long, C.c_double, C.c_void_p, C.c_long, C.c_long, C.c_void_p, C.c_long, C.c_long, C.c_int]),
    "target_manager_population_tick": (C.c_int, [C.c_void_p]),
    # one manager over several devices
    "target_manager_set_devices": (C.c_int, [C.c_void_p, C.POINTER(C.c_int), C.c_int]),
    "target_manager_num_shards": (C.c_int, [C.c_void_p]),
    "target_manager_shard_device": (C.c_int, [C.c_void_p, C.c_int]),
    "target_manager_shard_of": (C.c_int, [C.c_void_p, C.c_uint]),
    "target_manager_batch_shard": (C.c_int, [C.c_void_p, C.c_int]),
    "target_manager_set_shard_stream": (C.c_int, [C.c_void_p, C.c_int, C.c_void_p]),
    "target_manager_get_est_all_by_id": (C.c_long, [C.c_void_p, C.c_void_p, C.c_long]),
    "target_manager_step_sequence_all": (C.c_int, [C.c_void_p, C.c_long, C.c_double, C.c_void_p, C.c_long, C.c_int, c_double_p, C.c_double, C.c_int]),
    "target_batch_step_fused": (C.c_int, [C.c_void_p, C.c_long, C.c_double, C.c_void_p, C.c_long, C.c_long, C.c_void_p, C.c_long]),
    "target_batch_step_sequence_poses": (C.c_int, [C.c_void_p, C.c_long, C.c_double, C.c_void_p, C.c_long, C.c_long, C.c_void_p, C.c_long,
                                                   C.c_long, C.POINTER(PoseStream), C.c_int]),
    "target_batch_step_fused_poses": (C.c_int, [C.c_void_p, C.c_long, C.c_double, C.c_void_p, C.c_long, C.c_long, C.c_void_p, C.c_long,
                                                C.POINTER(PoseStream)]),
    "target_manager_step_sequence_all_poses": (C.c_int, [C.c_void_p, C.c_long, C.c_double, C.c_void_p, C.POINTER(PoseStream), C.c_long,
                                                         C.c_int, c_double_p, C.c_double, C.c_int]),
    "target_batch_step_sequence_innov": (C.c_int, [C.c_void_p, C.c_long, C.c_double, C.c_void_p, C.c_long, C.c_long, C.c_void_p, C.c_long,
                                                   C.c_long, C.POINTER(PoseStream), C.POINTER(InnovStream), C.c_int]),
    "target_manager_step_sequence_all_innov": (C.c_int, [C.c_void_p, C.c_long, C.c_double, C.c_void_p, C.POINTER(PoseStream),
                                                         C.POINTER(InnovStream), C.c_long, C.c_int, c_double_p, C.c_double, C.c_int]),
    "target_batch_step_sequence_gated": (C.c_int, [C.c_void_p, C.c_long, C.c_double, C.c_void_p, C.c_long, C.c_long, C.c_void_p, C.c_long,
                                                   C.c_long, C.POINTER(PoseStream), C.POINTER(InnovStream), C.c_double, C.c_int]),
    "target_manager_step_sequence_all_gated": (C.c_int, [C.c_void_p, C.c_long, C.c_double, C.c_void_p, C.POINTER(PoseStream),
                                                         C.POINTER(InnovStream), c_double_p, C.c_long, C.c_int, c_double_p, C.c_double,
                                                         C.c_int]),
    "target_batch_step_sequence_reacquire": (C.c_int, [C.c_void_p, C.c_long, C.c_double, C.c_void_p, C.c_long, C.c_long, C.c_void_p, C.c_long,
                                                       C.c_long, C.POINTER(PoseStream), C.POINTER(InnovStream), C.c_double, C.POINTER(Reacquire),
                                                       C.c_int]),
    "target_manager_step_sequence_all_reacquire": (C.c_int, [C.c_void_p, C.c_long, C.c_double, C.c_void_p, C.POINTER(PoseStream),
                                                             C.POINTER(InnovStream), c_double_p, C.POINTER(Reacquire), C.c_long, C.c_int,
                                                             c_double_p, C.c_double, C.c_int]),
    "target_batch_step_fused_gated": (C.c_int, [C.c_void_p, C.c_long, C.c_double, C.c_void_p, C.c_long, C.c_long, C.c_void_p, C.c_long,
                                                C.POINTER(PoseStream), C.POINTER(InnovStream), C.c_double, C.POINTER(Reacquire)]),
    "target_batch_step_fused_gate_served": (C.c_int, [C.c_void_p]),
    # a time step per tick (dt_host [n_ticks] in place of dt)
    "target_batch_step_sequence_dt": (C.c_int, [C.c_void_p, C.c_long, c_double_p, C.c_void_p, C.c_long, C.c_long, C.c_void_p, C.c_long,
                                                C.c_long, C.POINTER(PoseStream), C.POINTER(InnovStream), C.c_double, C.POINTER(Reacquire),
                                                C.c_int]),
    "target_batch_step_fused_dt": (C.c_int, [C.c_void_p, C.c_long, c_double_p, C.c_void_p, C.c_long, C.c_long, C.c_void_p, C.c_long,
                                             C.POINTER(PoseStream), C.POINTER(InnovStream), C.c_double, C.POINTER(Reacquire)]),
    "target_batch_step_fused_dt_served": (C.c_int, [C.c_void_p, C.c_int]),
    "target_manager_step_sequence_all_dt": (C.c_int, [C.c_void_p, C.c_long, c_double_p, C.c_void_p, C.POINTER(PoseStream),
                                                      C.POINTER(InnovStream), c_double_p, C.POINTER(Reacquire), C.c_long, C.c_int,
                                                      c_double_p, C.c_double, C.c_int]),
    # one launch for a temporally fused replay of a whole manager
    "target_manager_step_fused_all": (C.c_int, [C.c_void_p, C.c_long, C.c_double, C.c_void_p, C.POINTER(PoseStream), C.POINTER(InnovStream),
                                                c_double_p, C.POINTER(Reacquire), C.c_long]),
    "target_manager_step_fused_all_dt": (C.c_int, [C.c_void_p, C.c_long, c_double_p, C.c_void_p, C.POINTER(PoseStream), C.POINTER(InnovStream),
                                                   c_double_p, C.POINTER(Reacquire), C.c_long]),
    "target_manager_step_fused_all_served": (C.c_int, [C.c_void_p, C.c_int, C.c_int]),
    "target_batch_graph_recordings": (C.c_long, [C.c_void_p]),
    "target_batch_rejection_runs": (C.c_int, [C.c_void_p, C.c_void_p]),
    "target_manager_get_rejection_run": (C.c_int, [C.c_void_p, C.c_uint]),
    "target_manager_set_update_gate": (C.c_int, [C.c_void_p, C.c_int, C.c_double, C.c_int]),
    "target_manager_get_update_gate": (C.c_int, [C.c_void_p, C.c_int, c_double_p, C.POINTER(C.c_int)]),
    "target_manager_update_gate_served": (C.c_int, [C.c_void_p, C.c_int]),
    "target_manager_update_meas_batch_gated": (C.c_long, [C.c_void_p, c_uint_p, C.c_long, C.c_double, c_double_p, c_ubyte_p, c_double_p,
                                                         c_ubyte_p]),
    "target_batch_live_start": (C.c_int, [C.c_void_p, C.c_double, C.c_void_p, C.c_long, C.c_long, C.c_void_p, C.c_long, C.c_long, C.c_long,
                                          C.c_long, C.c_double]),
    "target_batch_live_set_pose_output": (C.c_int, [C.c_void_p, C.c_void_p, C.c_long]),
    "target_batch_live_set_gate": (C.c_int, [C.c_void_p, C.c_double, C.c_void_p, C.c_void_p]),
    "target_batch_live_gate_served": (C.c_int, [C.c_void_p]),
    "target_batch_live_post": (C.c_int, [C.c_void_p, C.c_long]),
    "target_batch_live_post_each": (C.c_int, [C.c_void_p, C.c_long]),
    "target_batch_live_done": (C.c_long, [C.c_void_p]),
    "target_batch_live_wait": (C.c_int, [C.c_void_p, C.c_long, C.c_double]),
    "target_batch_live_stop": (C.c_long, [C.c_void_p]),
    "target_batch_live_capacity": (C.c_long, [C.c_void_p]),
    "target_batch_live_running": (C.c_int, [C.c_void_p]),
    "target_manager_live_start_all": (C.c_int, [C.c_void_p, C.c_double, C.c_void_p, C.c_long, C.c_long, C.c_long, C.c_double, C.c_int,
                                                c_double_p, C.c_double]),
    "target_manager_live_post_all": (C.c_int, [C.c_void_p, C.c_long, C.c_int]),
    "target_manager_live_done_all": (C.c_long, [C.c_void_p]),
    "target_manager_live_wait_all": (C.c_int, [C.c_void_p, C.c_long, C.c_double]),
    "target_manager_live_stop_all": (C.c_long, [C.c_void_p]),
    "target_batch_get_est_dev": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_double]),
    "target_stream_fill_dev": (C.c_int, [C.POINTER(StreamSpec), C.c_long, C.c_long, C.c_long, C.c_int, C.c_void_p, C.c_long, C.c_long,
                                         C.c_void_p, C.c_long, C.c_void_p]),
    "target_stream_truth_dev": (C.c_int, [C.POINTER(StreamSpec), C.c_long, C.c_void_p, C.c_void_p, C.c_void_p]),
    "target_batch_pack_meas_dev": (C.c_int, [C.c_void_p, C.c_void_p, C.c_long, C.c_void_p, C.c_long]),
}


def lib():
    """The loaded shared library; raises (loudly) if it has not been built."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB):
        raise RuntimeError(
            "target_estimation_amd: %s is missing. Build it with "
            "`python -c 'import __graft_entry__ as g; g.build()'` (hipcc, gfx950). "
            "There is no CPU fallback." % LIB)
    # One HIP runtime per process: torch wheels bundle their own libamdhip64.so (SONAME
    # libamdhip64.so.7, the same as /opt/rocm's).  If torch is imported first, the dynamic loader
    # resolves this library's DT_NEEDED against the copy already mapped; loaded the other way round
    # the process ends up with two runtimes and the second one finds no device.
    try:
        import torch  # noqa: F401
    except ImportError:
        pass
    handle = C.CDLL(LIB)
    for name, (restype, argtypes) in SIGNATURES.items():
        fn = getattr(handle, name)  # AttributeError if a declared symbol is not exported
        fn.restype = restype
        fn.argtypes = argtypes
    _lib = handle
    return _lib


def last_error():
    return lib().target_manager_last_error().decode()
