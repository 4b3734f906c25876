"""The C-ABI library loads and exports exactly what include/qspec_hip.h declares (no GPU needed)."""
import ctypes
import os
import re

import pytest

from qspec_amd import _lib


def test_library_is_built():
    assert os.path.exists(_lib.LIB_PATH), "run `python -c 'import __graft_entry__ as g; g.build()'`"


def test_header_and_binding_agree():
    assert _lib.header_symbols() == sorted(_lib.SIGNATURES)


def test_every_declared_symbol_is_exported():
    lib = ctypes.CDLL(_lib.LIB_PATH)
    for name in _lib.header_symbols():
        assert hasattr(lib, name), name


def test_load_binds_prototypes_and_reports_errors():
    lib = _lib.load()
    assert lib.qspec_abi_version() == 6
    # argument validation happens before any HIP call, so it is testable without a GPU
    rc = lib.qspec_rms_norm_general_fuse_sum_fp16(None, None, 1e-5, 4, 4096, None)
    assert rc != 0 and b"NULL" in lib.qspec_last_error()
    rc = lib.qspec_rowwise_scaled_linear_s4s4(1, 1, 1, 1, None, 1, 4, 100, 4096, None)
    assert rc != 0 and b"N % 16" in lib.qspec_last_error()
    with pytest.raises(_lib.QSpecLibraryError):
        _lib.check(rc, lib)


def _param_names():
    """entry -> its parameter names, as include/qspec_hip.h spells them"""
    text = re.sub(r"/\*.*?\*/", "", open(_lib.HEADER_PATH).read(), flags=re.S)
    return {name: [re.findall(r"\w+", p)[-1] for p in params.split(",")]
            for name, params in re.findall(r"\b(qspec_\w+)\s*\(([^;{()]*)\)\s*;", text) if params.strip() != "void"}


def _checked_entries():
    """Every entry that returns int and takes a pointer, minus the shape queries, the one-shot all-reduce (its handles are not
    NULL-checked arguments) and qspec_collect_error_words (all-NULL with clear != 0 is a valid call: it launches)."""
    def is_query(n):
        return n.endswith("_supported") or "_slices" in n or n.endswith("_grid")
    return sorted(n for n, (res, args) in _lib.SIGNATURES.items()
                  if res is ctypes.c_int and any(t is ctypes.c_void_p or t is ctypes.POINTER(ctypes.c_void_p) for t in args)
                  and not is_query(n) and not n.startswith("qspec_oneshot_") and n != "qspec_collect_error_words")


def _null_args(name):
    """every pointer NULL, every integer 4, every float 1.0"""
    return [1.0 if t is ctypes.c_float else 4 if t in (ctypes.c_int, ctypes.c_int64, ctypes.c_uint64, ctypes.c_size_t) else None
            for t in _lib.SIGNATURES[name][1]]


_SAMPLE = ("qspec_sample_top_k_top_p", "qspec_sample_top_k_top_p_min_p")
_SAMPLE_SEEDED = ("qspec_sample_top_k_top_p_seeded", "qspec_sample_top_k_top_p_min_p_seeded")
_REJECTION = ("qspec_rejection_sample", "qspec_rejection_sample_seeded")
_LOGITS = ("qspec_process_logits", "qspec_process_logits_constrained")
_SAMPLE_PTRS = ("logits", "probs", "token", "workspace", "seq_seeds", "seq_seeded", "base_pos")
_REJECTION_PTRS = ("target_with_bonus_probs", "bonus_token_ids", "draft_probs", "draft_token_ids", "out_tokens", "accepted",
                   "recovered", "workspace", "seq_seeds", "seq_seeded", "base_pos")
_LOGITS_PTRS = ("logits", "tok_table", "repetition", "frequency", "presence", "min_tokens", "gen_base", "gen_lens", "stop_ids",
                "num_stop_ids", "deny", "meta", "bias_ids", "bias_vals", "words", "word_lens", "tail", "gen_tokens")
# The range checks of the sampler entries, one per row: (entries, the pointers that get a host buffer, integers, message).  The
# rows build on the all-NULL vectors: the pointers that are tested in front of the check point at a small host buffer, the
# integers hit the check, and whatever can still refuse the call behind it does (qspec_process_logits*: draft_ids stays NULL with
# draft_rows = 4; the seeded samplers: draw_stream = 0), so that no row reaches a HIP call.  `out` of qspec_process_logits* gets
# a second buffer (logits == out is a check of its own).  The messages are those of the library before the entries shared
# their bodies.
_RANGE_ROWS = [
    (_SAMPLE + _SAMPLE_SEEDED, _SAMPLE_PTRS, {"vocab": 0, "rows_per_seq": 0}, "vocab < 1"),
    (_SAMPLE_SEEDED, _SAMPLE_PTRS, {"rows_per_seq": 0, "draw_stream": 0}, "rows_per_seq=0 must be >= 1"),
    (_SAMPLE_SEEDED, _SAMPLE_PTRS, {"num_seqs": 1, "rows_per_seq": 2, "draw_stream": 0},
     "num_seqs=1 x rows_per_seq=2 does not cover tokens=4"),
    (_SAMPLE_SEEDED, _SAMPLE_PTRS, {"j_base": -1, "draw_stream": 0}, "j_base=-1 + rows_per_seq=4 outside the 16-bit sub-index"),
    (_SAMPLE_SEEDED, _SAMPLE_PTRS, {"j_base": 65533, "draw_stream": 0},
     "j_base=65533 + rows_per_seq=4 outside the 16-bit sub-index"),
    (_SAMPLE_SEEDED, _SAMPLE_PTRS, {"draw_stream": 0}, "draw_stream=0 must be 1 (draft) or 2 (target)"),
    (_LOGITS, _LOGITS_PTRS + ("out=logits",), {}, "the pass is out of place (logits == out)"),
    (_LOGITS, _LOGITS_PTRS + ("out",), {"vocab": 0}, "vocab < 1"),
    (_LOGITS, _LOGITS_PTRS + ("out",), {"rows_per_seq": 0}, "rows_per_seq=0 must be >= 1"),
    (_LOGITS, _LOGITS_PTRS + ("out",), {"j_base": -1}, "j_base < 0"),
    (_LOGITS, _LOGITS_PTRS + ("out",), {"stop_ids_per_slot": -1}, "stop_ids_per_slot=-1 outside 0..16"),
    (_LOGITS, _LOGITS_PTRS + ("out",), {"stop_ids_per_slot": 17}, "stop_ids_per_slot=17 outside 0..16"),
    (_LOGITS[1:], _LOGITS_PTRS + ("out",), {"deny_words": 0}, "deny_words=0 does not cover vocab=4"),
    (_LOGITS[1:], _LOGITS_PTRS + ("out",), {"gen_cap": 0}, "gen_cap=0 must be >= 1"),
    (_REJECTION, _REJECTION_PTRS, {"batch": 1025}, "batch*k=4100 too large"),
    (_REJECTION, _REJECTION_PTRS, {"k": 0}, "k=0 must be >= 1"),
    (_REJECTION, _REJECTION_PTRS, {"k": -1}, "k=-1 must be >= 1"),
]


def _range_calls():
    """-> [(entry, args, message)] of _RANGE_ROWS; the buffers live as long as the list"""
    names = _param_names()
    bufs = [ctypes.create_string_buffer(64), ctypes.create_string_buffer(64)]
    p, p_out = (ctypes.cast(b, ctypes.c_void_p) for b in bufs)
    calls = []
    for entries, ptrs, ints, message in _RANGE_ROWS:
        for entry in entries:
            args = _null_args(entry)
            for i, n in enumerate(names[entry]):
                if n == "out" and "out=logits" in ptrs:
                    args[i] = p
                elif n in ptrs:
                    args[i] = p_out if n == "out" else p
                elif n in ints:
                    args[i] = ints[n]
            calls.append((entry, args, "%s: %s" % (entry, message)))
    return calls, bufs


def test_every_entry_refuses_bad_arguments_under_its_own_name():
    """Argument validation comes before any HIP call and names the entry that was called: every checked entry with all-NULL
    pointers, then the range checks of the sampler entries one by one (_RANGE_ROWS)."""
    lib = _lib.load()
    names = _param_names()
    entries = _checked_entries()
    assert {n + "_xp" for n in _lib.XP_TWINS} <= set(entries) and sum(n.endswith("_kv8") for n in entries) == 8
    assert all(len(names[n]) == len(_lib.SIGNATURES[n][1]) for n in entries)
    wrong = []
    for entry in entries:
        rc = getattr(lib, entry)(*_null_args(entry))
        err = lib.qspec_last_error().decode()
        if rc == 0 or not err.startswith(entry + ":") or "launch failed" in err:
            wrong.append((entry, rc, err))
    calls, _keep = _range_calls()
    for entry, args, message in calls:
        rc = getattr(lib, entry)(*args)
        err = lib.qspec_last_error().decode()
        if rc == 0 or err != message:
            wrong.append((entry, rc, err, message))
    assert not wrong, wrong


def test_ops_refuse_cpu_tensors():
    import torch
    from qspec_amd import ops
    x = torch.zeros(2, 4096, dtype=torch.float16)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ops.rms_norm_general_fuse_sum_fp16(torch.empty_like(x), x, 1e-5)
