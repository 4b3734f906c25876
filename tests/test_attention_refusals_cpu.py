"""Refusals of qspec_paged_attention / qspec_paged_attention_kv8: what the entry answers for arguments no kernel serves,
decided before any launch (attention.hip: attn_form, behind the C boundary's own checks), so that no GPU is needed.  The
pointers are never dereferenced.  One row per refusal at the smallest shape that triggers it; the expected answer is what
the library returned for the same arguments before the launch plan was gathered into attn_form -- the return value and
either the internal code the error string carries or the C boundary's own message.

Rows with a code are decided by attn_form.  The four rows without one (odd head size, head size above 256, no workspace,
head size 66 with an fp8 cache) are answered by the C boundary's own checks in front of it, so attn_form's -1 for those
head sizes and its -6 cannot be reached through the C API and are not pinned here."""
import ctypes
import re

import pytest

from qspec_amd import _lib

P = "ptr"   # a live pointer that is never dereferenced


def _row(id, *, kv8=False, n_seqs=1, max_q_len=1, nq=8, nkv=2, d=128, bs=16, max_blocks=4, n_splits=1, ws=P, out=P):
    return pytest.param(dict(kv8=kv8, n_seqs=n_seqs, max_q_len=max_q_len, nq=nq, nkv=nkv, d=d, bs=bs, max_blocks=max_blocks,
                             n_splits=n_splits, ws=ws, out=out), id=id)


# (arguments, return value, internal code or None, fragment of the error string)
ROWS = [
    (_row("heads-not-a-multiple-of-kv-heads", nq=3, nkv=2), 1, -1, "unsupported shape"),
    (_row("head-size-odd", d=127), 1, None, "head_size=127"),
    (_row("head-size-above-256", d=258), 1, None, "head_size=258"),
    (_row("splits-0-d128", n_splits=0), 1, -3, "unsupported shape"),
    (_row("splits-65-d128", n_splits=65), 1, -3, "unsupported shape"),
    (_row("splits-0-d64", d=64, n_splits=0), 1, -3, "unsupported shape"),
    (_row("splits-65-d64", d=64, n_splits=65), 1, -3, "unsupported shape"),
    (_row("no-out-no-workspace-d64", d=64, ws=None, out=None), 1, None, "`workspace` is NULL"),
    (_row("block-size-24", bs=24), 1, -5, "unsupported shape"),
    (_row("gqa-group-3", nq=6, nkv=2), 1, -5, "unsupported shape"),
    # in-kernel merge: one ticket counter per (sequence, kv head, row block), 4096 of them
    (_row("merged-above-4096-counters", n_seqs=4097, nq=1, nkv=1, n_splits=2), 1, -4, "unsupported shape"),
    (_row("head-size-66-fp8", kv8=True, d=66), 1, None, "no fp8 form"),
    # The scores of one split must fit 64 KiB of LDS: 1025 blocks of 16 keys = 16400 keys > 16384.  The one row whose code is
    # NOT a recorded answer: before attn_form this check sat behind the LDS opt-in, a runtime call that fails without a GPU
    # (code -8 there); -2 is what the source of that version returns once the call succeeds.
    (_row("scores-above-the-lds-cap-d64", d=64, max_blocks=1025), 1, -2, "unsupported shape"),
    (_row("no-sequences", n_seqs=0), 0, None, ""),
]


@pytest.mark.parametrize("args,rc,code,text", [(r[0].values[0], *r[1:]) for r in ROWS], ids=[r[0].id for r in ROWS])
def test_paged_attention_refusal(args, rc, code, text):
    lib = _lib.load()
    buf = ctypes.create_string_buffer(64)
    live = ctypes.cast(buf, ctypes.c_void_p)
    ptr = lambda v: live if v == P else None
    tokens = args["n_seqs"] * args["max_q_len"]
    head = (live, 0, live, live) + ((1.0, 1.0) if args["kv8"] else ())
    fn = lib.qspec_paged_attention_kv8 if args["kv8"] else lib.qspec_paged_attention
    got = fn(*head, live, args["max_blocks"], live, live, args["n_seqs"], tokens, args["max_q_len"], args["nq"], args["nkv"],
             args["d"], args["bs"], 0.1, args["n_splits"], ptr(args["ws"]), ptr(args["out"]), None)
    err = lib.qspec_last_error().decode() if got else ""
    m = re.search(r"\(code (-?\d+)\)", err)
    assert (got, int(m.group(1)) if m else None) == (rc, code), err
    assert text in err, err
