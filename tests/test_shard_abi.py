"""The C ABI of a manager over several devices (target_manager_set_devices and its introspection calls, and
target_manager_get_est_all_by_id): declared in the header, exported by the library, prototyped in capi.py.  No GPU."""
import os
import re

from conftest import ROOT

NEW = ["target_manager_set_devices", "target_manager_num_shards", "target_manager_shard_device", "target_manager_shard_of",
       "target_manager_batch_shard", "target_manager_set_shard_stream", "target_manager_get_est_all_by_id"]


def test_shard_symbols_declared_exported_and_bound():
    from target_estimation_amd import capi
    text = open(os.path.join(ROOT, "include", "target_estimation_amd", "target_batch_c.h")).read()
    code = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    lib = capi.lib()
    for name in NEW:
        assert re.search(r"\b%s\s*\(" % name, code), "not declared: %s" % name
        assert hasattr(lib, name), "not exported: %s" % name
        assert name in capi.SIGNATURES, "not prototyped: %s" % name


def test_header_states_the_refusals():
    text = open(os.path.join(ROOT, "include", "target_estimation_amd", "target_batch_c.h")).read()
    block = text[text.index("target_manager_set_devices"):text.index("int target_manager_set_devices")]
    for what in ("target_manager_live_*_all", "target_manager_gather_pose_*", "target_manager_set_stream", "REFUSED"):
        assert what in block


def test_null_handles_of_the_shard_calls():
    from target_estimation_amd import capi
    lib = capi.lib()
    assert lib.target_manager_set_devices(None, None, 1) == -1
    assert lib.target_manager_num_shards(None) == -1
    assert lib.target_manager_shard_device(None, 0) == -1
    assert lib.target_manager_shard_of(None, 1) == -1
    assert lib.target_manager_batch_shard(None, 0) == -1
    assert lib.target_manager_set_shard_stream(None, 0, None) == -1
    assert lib.target_manager_get_est_all_by_id(None, None, 0) == -1
    assert b"NULL manager handle" in lib.target_manager_last_error()
