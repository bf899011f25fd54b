"""The duplicate-track search at the C boundary and in the Python front end (no GPU needed): the two symbols are exported, declared
in target_batch_c.h and bound in capi.py with the header's prototypes and struct; the header carries the contract; what does not
depend on a handle is refused before the handle is looked at, and a NULL handle is an error, not a crash."""
import ctypes as C
import inspect
import os
import re

from conftest import ROOT

HEADER = os.path.join(ROOT, "include", "target_estimation_amd", "target_batch_c.h")
NEW = {"target_manager_find_duplicates_dev": "int", "target_manager_retire_duplicates": "int"}
NAN, INF = float("nan"), float("inf")


def _decl(text, name, res):
    m = re.search(r"\b%s\s+%s\s*\((.*?)\)\s*;" % (res, name), text, flags=re.S)
    assert m, "not declared: %s %s" % (res, name)
    return [a.strip() for a in re.sub(r"\s+", " ", m.group(1)).split(",")]


def test_exported_declared_and_bound():
    from target_estimation_amd import capi
    lib = capi.lib()
    whole = open(HEADER).read()
    text = re.sub(r"/\*.*?\*/", "", whole, flags=re.S)
    scalar = {"long": C.c_long, "double": C.c_double, "int": C.c_int}
    host = {"const target_dup_out_c* per_batch": C.POINTER(capi.DupOut), "unsigned int* retired_ids_out": capi.c_uint_p,
            "unsigned int* kept_ids_out": capi.c_uint_p, "long* info": C.POINTER(C.c_long)}
    for name, res in NEW.items():
        assert hasattr(lib, name), "not exported: %s" % name
        args = _decl(text, name, res)
        restype, sig = capi.SIGNATURES[name]
        assert restype is scalar[res] and len(sig) == len(args), (name, args)
        for a, c in zip(args, sig):
            if "*" in a:
                assert c is host.get(a, C.c_void_p), (name, a)
            else:
                assert c is scalar[a.rsplit(" ", 1)[0]], (name, a)
    assert _decl(text, "target_manager_find_duplicates_dev", "int") == [
        "target_manager_c* m", "double dt", "double gate", "int rounds", "double cell", "int min_hits", "const target_dup_out_c* per_batch",
        "long n_batches", "int* info_dev"]
    assert _decl(text, "target_manager_retire_duplicates", "int") == [
        "target_manager_c* m", "double dt", "double gate", "int rounds", "double cell", "int min_hits", "unsigned int* retired_ids_out",
        "unsigned int* kept_ids_out", "long cap", "long* info"]
    m = re.search(r"typedef struct target_dup_out_c \{(.*?)\} target_dup_out_c;", text, flags=re.S)
    fields = [f.strip().rsplit(" ", 1) for f in m.group(1).split(";") if f.strip()]
    assert [(n, C.c_void_p) for t, n in fields] == list(capi.DupOut._fields_) and all("*" in t for t, n in fields)
    assert [n for t, n in fields] == ["dup_out_dev", "partner_batch_dev", "partner_slot_dev", "d2_of_slot_dev"]


def test_header_carries_the_contract():
    whole = open(HEADER).read()
    section = whole[whole.index("DUPLICATE TRACKS"):whole.index("typedef struct target_dup_out_c")]
    section = re.sub(r"\s*\n \*\s*", " ", section)   # (the comment's line breaks are not part of the contract)
    for phrase in ("row against row", "target_manager_get_batch order", "BEFORE it adds R", "one validity rule", ">= min_hits (0 .. 255)",
                   "NARROW", "EXCLUDED, not brute-forced", "counted in info[3]", "cell is too small", "C = Sigma_lo + Sigma_hi",
                   "an invalid C rejects the pair", "27 cells suffice", "both order the pair as (lo, hi)", "(d2, partner row)", "never itself",
                   "TARGET_ASSOC_MAX_ROUNDS", "sorted greedy matching by (d2, lo, hi)", "fewer hits; at equal hits, more miss; at equal both, the higher row",
                   "loses one track per call", "function of the inputs alone", "allocates nothing", "never waits on the host",
                   "{pairs, rounds_run, settled, wide rows}", "{0, 0, 1, 0}", "BEFORE anything moves", "ascending former slot",
                   "{retired, rounds_run, settled, wide}", "WAITS ON THE HOST", "NOT CAPTURABLE",
                   "recorded sequences, uniform tiles, shared-axes batches and live sessions", "bit for bit", "STALE afterwards",
                   "NOTHING CHANGES on a refusal", "before the handle is looked at", "Not built", "fusing the two estimates",
                   "brute force for wide rows", "several shards", "orientation", "the Eigen facade"):
        assert phrase in section, phrase
    # the plan header carries the two arguments the contract rests on
    plan = open(os.path.join(ROOT, "target_estimation_amd", "csrc", "track_merge_plan.hpp")).read()
    plan = re.sub(r"\s*\n//\s*", " ", plan)
    for phrase in ("exactly", "rounding is monotone", "never exceeds the larger of the two rows' reach2", "27 cells",
                   "smallest remaining pair is always mutual", "EXCLUDED", "`cell` is too small"):
        assert phrase in plan, phrase


def test_python_signatures():
    import target_estimation_amd as te
    p = inspect.signature(te.TargetManager.find_duplicates).parameters
    assert list(p) == ["self", "dt", "gate", "cell", "rounds", "min_hits", "out"]
    assert p["rounds"].default == 8 and p["min_hits"].default == 1 and p["out"].default is None
    p = inspect.signature(te.TargetManager.retire_duplicates).parameters
    assert list(p) == ["self", "dt", "gate", "cell", "rounds", "min_hits"]
    assert p["rounds"].default == 8 and p["min_hits"].default == 1


def test_refusals_come_before_the_handle_and_null_handles_are_errors():
    from target_estimation_amd import capi
    lib = capi.lib()
    P = 4096          # a non-NULL pointer that is never dereferenced: every call below is refused first
    per = (capi.DupOut * 2)()
    ids = (C.c_uint * 4)()
    info = (C.c_long * 4)()
    # find: (dt, gate, rounds, cell, min_hits, per_batch, n_batches, info_dev)
    good = [0.01, 9.0, 4, 0.5, 1, per, 2, P]
    table = [({7: None}, "info is required"), ({0: -0.01}, "dt must be >= 0"), ({0: NAN}, "dt must be >= 0"),
             ({1: 0.0}, "gate must be > 0 and finite"), ({1: -1.0}, "gate must be > 0 and finite"), ({1: NAN}, "gate must be > 0 and finite"),
             ({1: INF}, "gate must be > 0 and finite"), ({2: 0}, "rounds must be 1..16"), ({2: 17}, "rounds must be 1..16"),
             ({3: 0.0}, "cell must be > 0 and finite"), ({3: -2.0}, "cell must be > 0 and finite"), ({3: NAN}, "cell must be > 0 and finite"),
             ({3: INF}, "cell must be > 0 and finite"), ({4: -1}, "min_hits must be 0..255"), ({4: 256}, "min_hits must be 0..255"),
             ({6: -1}, "one output description per batch"), ({5: None}, "one output description per batch"),
             ({}, "NULL manager handle"), ({4: 0}, "NULL manager handle"), ({4: 255, 2: 16}, "NULL manager handle"),
             ({5: None, 6: 0}, "NULL manager handle")]
    for change, why in table:
        args = list(good)
        for k, v in change.items():
            args[k] = v
        assert lib.target_manager_find_duplicates_dev(None, *args) == -1, why
        assert why in capi.last_error() and "target_manager_find_duplicates_dev" in capi.last_error(), (why, capi.last_error())
    # retire: (dt, gate, rounds, cell, min_hits, retired, kept, cap, info)
    good = [0.01, 9.0, 4, 0.5, 1, ids, ids, 4, info]
    table = [({8: None}, "info is required"), ({0: -0.01}, "dt must be >= 0"), ({0: NAN}, "dt must be >= 0"),
             ({1: 0.0}, "gate must be > 0 and finite"), ({1: NAN}, "gate must be > 0 and finite"), ({1: INF}, "gate must be > 0 and finite"),
             ({2: 0}, "rounds must be 1..16"), ({2: 17}, "rounds must be 1..16"), ({3: 0.0}, "cell must be > 0 and finite"),
             ({3: NAN}, "cell must be > 0 and finite"), ({3: INF}, "cell must be > 0 and finite"), ({4: -1}, "min_hits must be 0..255"),
             ({4: 256}, "min_hits must be 0..255"), ({7: -1}, "required for cap > 0"), ({5: None}, "required for cap > 0"),
             ({6: None}, "required for cap > 0"), ({}, "NULL manager handle"), ({5: None, 6: None, 7: 0}, "NULL manager handle")]
    for change, why in table:
        args = list(good)
        for k, v in change.items():
            args[k] = v
        assert lib.target_manager_retire_duplicates(None, *args) == -1, why
        assert why in capi.last_error() and "target_manager_retire_duplicates" in capi.last_error(), (why, capi.last_error())
