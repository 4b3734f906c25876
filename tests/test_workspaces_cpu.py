"""The per-stream workspace registry of qspec_amd/ops.py on the host (no GPU): one cache keyed by (kind, device, stream
[, rows]), one table of sticky error-word positions, and the thread-local switch that recovery replays use.  The stream id
and the library's size functions are replaced by controllable stubs; the tensors live on the CPU."""
import threading
from types import SimpleNamespace

import pytest
import torch

from qspec_amd import _lib, ops

DEV = torch.device("cpu", 0)
BYTES = {"xwg": 256, "ln": 192, "w4a16": 96}          # fixed-size kinds
ROW_BYTES = {"sampler": 24, "lm_head": 40, "sample": 56}   # bytes per row of the row-sized kinds
ZEROED = ("xwg", "ln", "w4a16", "sample")


@pytest.fixture
def stream(monkeypatch):
    """An empty registry, a stub library and a stream id the test sets through `stream.id`."""
    cur = SimpleNamespace(id=7)
    lib = SimpleNamespace(qspec_xwg_workspace_bytes=lambda: BYTES["xwg"],
                          qspec_ln_linear_workspace_bytes=lambda: BYTES["ln"],
                          qspec_w4a16_workspace_bytes=lambda: BYTES["w4a16"],
                          qspec_sampler_workspace_bytes=lambda rows: ROW_BYTES["sampler"] * rows,
                          qspec_lm_head_sampler_workspace_bytes=lambda rows: ROW_BYTES["lm_head"] * rows,
                          qspec_sample_workspace_bytes=lambda rows: ROW_BYTES["sample"] * rows)
    monkeypatch.setattr(_lib, "load", lambda: lib)
    monkeypatch.setattr(ops, "_stream_id", lambda device: cur.id)
    monkeypatch.setattr(ops, "_workspaces", {})
    monkeypatch.setattr(ops, "XWG_SPREAD", True)
    monkeypatch.setattr(ops, "LN_HANDOFF", True)
    monkeypatch.setattr(ops, "LN_HANDOFF_MIN_M", 8)
    return cur


def _get(kind, rows=None):
    return ops._workspace(kind, DEV, rows=rows)


@pytest.mark.parametrize("kind", sorted(BYTES) + sorted(ROW_BYTES))
def test_cached_per_kind_device_stream_and_rows(stream, kind):
    rows = 3 if kind in ROW_BYTES else None
    ws = _get(kind, rows)
    assert _get(kind, rows) is ws
    nbytes = BYTES[kind] if rows is None else ROW_BYTES[kind] * rows
    if kind == "xwg":
        assert ws.dtype == torch.int32 and ws.shape == (nbytes // 4,)
    else:
        assert ws.dtype == torch.uint8 and ws.shape == (nbytes,)
    if kind in ZEROED:
        assert not ws.any()
    stream.id = 8
    other = _get(kind, rows)
    assert other is not ws and _get(kind, rows) is other
    stream.id = 7
    assert _get(kind, rows) is ws
    if rows is not None:
        more = _get(kind, rows + 1)
        assert more is not ws and more.numel() == ROW_BYTES[kind] * (rows + 1)
    assert all(_get(k, 3 if k in ROW_BYTES else None) is not ws for k in list(BYTES) + list(ROW_BYTES) if k != kind)


def test_rows_belong_to_the_row_sized_kinds_only(stream):
    with pytest.raises(AssertionError):
        _get("xwg", 3)
    with pytest.raises(AssertionError):
        _get("sample")


def test_public_helpers_go_through_the_registry(stream):
    assert ops.xwg_workspace(DEV) is _get("xwg") and ops.w4a16_workspace(DEV) is _get("w4a16")
    assert ops.ln_linear_workspace(DEV) is _get("ln")
    assert ops.sample_workspace(5, DEV) is _get("sample", 5)
    assert ops._sampler_ws(5, DEV) is _get("sampler", 5)
    mine = torch.zeros(1)
    assert ops._sampler_ws(5, DEV, mine) is mine
    private = ops.new_sample_workspace(5, DEV)
    assert private is not _get("sample", 5) and private.dtype == torch.uint8 and private.numel() == ROW_BYTES["sample"] * 5
    assert not private.any() and ops.new_sample_workspace(5, DEV) is not private


def test_ln_handoff_min_m_gate(stream):
    assert ops.ln_linear_workspace(DEV, 4) is None and ops.ln_linear_workspace(DEV, 7) is None
    ws = ops.ln_linear_workspace(DEV, 8)
    assert ws is not None and ops.ln_linear_workspace(DEV, 16) is ws and ops.ln_linear_workspace(DEV) is ws


def test_monkeypatched_defaults_switch_the_workspaces_off(stream, monkeypatch):
    monkeypatch.setattr(ops, "XWG_SPREAD", False)
    assert ops.xwg_workspace(DEV) is None and ops.ln_linear_workspace(DEV, 16) is not None
    monkeypatch.setattr(ops, "LN_HANDOFF", False)
    assert ops.ln_linear_workspace(DEV, 16) is None


def _handoff_workspaces(stream, ids=(7, 8)):
    made = []
    for i in ids:
        stream.id = i
        made.append((ops.xwg_workspace(DEV), ops.ln_linear_workspace(DEV, 16)))
        ops.w4a16_workspace(DEV), ops.sample_workspace(2, DEV)   # kinds without an error word
    return made


def test_error_words_alias_word_0_and_word_31(stream):
    made = _handoff_workspaces(stream)
    for n, (xwg, ln) in enumerate(made):
        xwg[0] = 100 + n
        ln.view(torch.int32)[31] = 200 + n
    words = ops.error_words(DEV)
    assert all(w.dtype == torch.int32 and w.shape == (1,) for w in words)
    assert sorted(int(w) for w in words) == [100, 101, 200, 201]
    stream.id = 8
    assert sorted(int(w) for w in ops.error_words(DEV, current_stream_only=True)) == [101, 201]
    assert sorted(ops.stream_error_words(DEV, extra=(0, 4096))) == sorted(
        [made[1][0].data_ptr(), made[1][1].data_ptr() + 31 * 4, 4096])
    assert sorted(ops.xwg_error_word(DEV).tolist()) == [100, 101]
    stream.id = 9   # a stream without workspaces; another device index
    assert ops.error_words(DEV, current_stream_only=True) == [] and ops.stream_error_words(DEV) == []
    assert ops.error_words(torch.device("cpu", 1)) == [] and ops.xwg_error_word(torch.device("cpu", 1)) is None


def test_clear_error_words_zeroes_exactly_those_words(stream):
    made = _handoff_workspaces(stream)
    others = [ws for key, ws in ops._workspaces.items() if key[0] not in ("xwg", "ln")]
    assert len(others) == 4
    for ws in [w for pair in made for w in pair] + others:
        ws.fill_(1)
    ops.clear_error_words(DEV)   # every stream of the device, whichever is current
    for xwg, ln in made:
        expect = torch.ones_like(xwg)
        expect[0] = 0
        assert torch.equal(xwg, expect)
        expect = torch.ones_like(ln).view(torch.int32)
        expect[31] = 0
        assert torch.equal(ln.view(torch.int32), expect)
    assert all(bool((ws == 1).all()) for ws in others)


def test_no_handoffs_restores_on_exit_on_error_and_nests(stream):
    xwg, ln = ops.xwg_workspace(DEV), ops.ln_linear_workspace(DEV, 16)

    def off():
        return ops.xwg_workspace(DEV) is None and ops.ln_linear_workspace(DEV, 16) is None

    def on():
        return ops.xwg_workspace(DEV) is xwg and ops.ln_linear_workspace(DEV, 16) is ln
    with ops.no_handoffs():
        assert off() and ops.XWG_SPREAD is True and ops.LN_HANDOFF is True
        assert ops.w4a16_workspace(DEV) is not None   # only the hand-off workspaces are switched
    assert on()
    with pytest.raises(ValueError):
        with ops.no_handoffs():
            assert off()
            raise ValueError("inside")
    assert on()
    with ops.no_handoffs():
        with ops.no_handoffs():
            assert off()
        assert off()
        with pytest.raises(ValueError):
            with ops.no_handoffs():
                raise ValueError("nested")
        assert off()
    assert on()


def test_no_handoffs_holds_on_the_calling_thread_only(stream):
    inside, checked = threading.Event(), threading.Event()
    seen = {}

    def first():
        with ops.no_handoffs():
            seen["first"] = (ops.xwg_workspace(DEV), ops.ln_linear_workspace(DEV, 16))
            inside.set()
            checked.wait(10)
        seen["first_after"] = (ops.xwg_workspace(DEV), ops.ln_linear_workspace(DEV, 16))

    def second():
        inside.wait(10)
        seen["second"] = (ops.xwg_workspace(DEV), ops.ln_linear_workspace(DEV, 16))
        checked.set()
    t1 = threading.Thread(target=first)
    t1.start()
    assert inside.wait(10)
    t2 = threading.Thread(target=second)   # started while the first thread is inside no_handoffs()
    t2.start()
    t2.join(10)
    t1.join(10)
    assert not t1.is_alive() and not t2.is_alive()
    assert seen["first"] == (None, None)
    assert all(w is not None for w in seen["second"])
    assert seen["first_after"][0] is seen["second"][0] and seen["first_after"][1] is seen["second"][1]
