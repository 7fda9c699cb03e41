"""The guard-band arena (tests/guard_arena.py) rejects what it is meant to reject, shown without a GPU, and the coverage
table: every entry point of include/cdvslam_hip.h that writes device memory is audited by tests/test_bounds_audit.py or is
exempt for one of the permitted reasons."""
import os
import re

import numpy as np
import pytest
import torch

from tests import guard_arena as GA

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _arena(which="A", row_bytes=0):
    a = GA.Arena("cpu", which, row_bytes, capacity=1 << 18)
    x = a.tensor("x", np.arange(7, dtype=np.float32))
    h = a.tensor("h", np.ones(882, np.float16))
    i = a.tensor("i", np.array([5], np.int64), index_max=9)
    return a, x, h, i


def test_carve_alignment_and_flush_ends():
    for which in ("A", "B"):
        a, x, h, i = _arena(which)
        base = a.buf.data_ptr()
        for t, name, nbytes in ((x, "x", 28), (h, "h", 1764), (i, "i", 8)):
            assert t.data_ptr() % 256 == 0
            s, e = a.span(name)
            assert base + s == t.data_ptr() and e - s == nbytes       # the tensor ends where the data ends ...
            back = a.buf[e:e + a.guard].numpy()
            front = a.buf[s - a.guard:s].numpy()
            assert a.guard >= 4096 and len(back) == a.guard           # ... and a whole guard follows and precedes it
            if name == "i":
                want = 0 if which == "A" else 9
                assert (back.view(np.int64) == want).all() and (front.view(np.int64) == want).all()
            elif which == "B":
                assert not back.any() and not front.any()
            else:
                ut = np.uint32 if name == "x" else np.uint16
                usable = back[: len(back) // np.dtype(ut).itemsize * np.dtype(ut).itemsize].view(ut)
                bits = GA.F32_NAN if name == "x" else GA.F16_NAN ^ 1      # the payload's low bits carry the tensor's number
                assert (usable == bits).all() and np.isnan(usable.view(np.float32 if name == "x" else np.float16)).all()
        assert x.tolist() == list(range(7)) and int(i[0]) == 5
        a.check()
    assert GA.guard_bytes(0) == 4096 and GA.guard_bytes(882 * 2) == 4096 and GA.guard_bytes(10368) == 10752
    assert GA.guard_bytes(10368) >= 10368 + 256


def test_index_guards_are_always_valid_indices():
    with pytest.raises(AssertionError):
        GA.guard_pattern(torch.int64, 64, "B", index_max=-1)
    with pytest.raises(AssertionError):
        GA.guard_pattern(torch.int64, 64, "B", index_max=2 ** 40)
    assert not GA.guard_pattern(torch.int64, 64, "A", index_max=7).any()
    assert (GA.guard_pattern(torch.int32, 64, "B", index_max=7).view(np.int32) == 7).all()


@pytest.mark.parametrize("name,side,where", [("x", "back", 0), ("h", "front", -1), ("i", "back", "far"), ("h", "back", 0),
                                              ("x", "front", "far")])
def test_planted_byte_is_reported_with_tensor_and_side(name, side, where):
    a, x, h, i = _arena()
    s, e = a.span(name)
    g = a.guard
    if side == "back":
        pos, dist = (e, 1) if where == 0 else (e + g - 1, g)
    else:
        pos, dist = (s - 1, 1) if where == -1 else (s - g, g)
    a.buf[pos] = int(a.buf[pos]) ^ 0x10
    d = a.first_difference()
    assert d[:3] == (name, side, dist)
    with pytest.raises(GA.GuardError) as ei:
        a.check("planted")
    msg = str(ei.value)
    assert "'%s'" % name in msg and side + " side" in msg and "%d byte(s)" % dist in msg


def _scale_rows(a, n, rows_written, read_past=0):
    """a numpy 'kernel': y[r] = 2 x[r] + sum of the `read_past` elements behind x's row block, for r < rows_written"""
    x = a.tensor("x", np.arange(n * 4, dtype=np.float32).reshape(n, 4))
    y = a.tensor("y", (n, 4), torch.float32)
    s, e = a.span("x")
    raw_x = a.buf[s:e + 4 * read_past].numpy().view(np.float32)       # the kernel's view of memory: no bounds
    ys, _ = a.span("y")
    raw_y = a.buf[ys:ys + 16 * rows_written].numpy().view(np.float32)
    extra = raw_x[n * 4:].sum() if read_past else np.float32(0)
    for r in range(rows_written):
        src = raw_x[4 * r:4 * r + 4] if r < n else np.zeros(4, np.float32)
        raw_y[4 * r:4 * r + 4] = 2 * src + (extra if r == n - 1 else 0)
    return {"y": y}


def test_fake_kernel_one_row_too_many_is_rejected():
    out = GA.run_twice(lambda a: _scale_rows(a, 5, 5), "cpu", row_bytes=16, capacity=1 << 16)
    assert np.array_equal(out["y"].numpy(), 2 * np.arange(20, dtype=np.float32).reshape(5, 4))
    with pytest.raises(GA.GuardError) as ei:
        GA.run_twice(lambda a: _scale_rows(a, 5, 6), "cpu", row_bytes=16, capacity=1 << 16, what="scale")
    assert "'y'" in str(ei.value) and "back side" in str(ei.value)


def test_fake_kernel_reading_one_element_past_its_input_is_rejected():
    """the rows are 'right' in pass B (zero guards) and NaN in pass A: only the comparison of the passes sees it"""
    with pytest.raises(GA.GuardError) as ei:
        GA.run_twice(lambda a: _scale_rows(a, 5, 5, read_past=1), "cpu", row_bytes=16, capacity=1 << 16, what="scale")
    assert "'y'" in str(ei.value) and "pass A and pass B" in str(ei.value)
    b = GA.Arena("cpu", "B", 16, 1 << 16)
    assert np.array_equal(_scale_rows(b, 5, 5, read_past=1)["y"].numpy(), 2 * np.arange(20, dtype=np.float32).reshape(5, 4))


def test_fake_gather_with_an_index_read_past_the_list_is_rejected():
    """an index list read one entry too far: guard 0 in pass A, the last valid row in pass B -- both in bounds, different"""
    def fn(a):
        table = np.arange(10, dtype=np.float32) + 1
        idx = a.tensor("idx", np.array([3, 9, 0], np.int64), index_max=9)
        out = a.tensor("out", (1,), torch.float32)
        s, e = a.span("idx")
        raw = a.buf[s:e + 8].numpy().view(np.int64)      # four entries instead of three
        assert 0 <= raw.min() and raw.max() <= 9
        out[0] = float(table[raw].sum())
        return {"out": out}
    with pytest.raises(GA.GuardError):
        GA.run_twice(fn, "cpu", capacity=1 << 16)


# ---------------------------------------------------------------------------------------------------
# coverage table
# ---------------------------------------------------------------------------------------------------

def _writers():
    """declared functions with a non-const pointer parameter that is device memory (not the stream handle, not *_host)"""
    src = open(os.path.join(ROOT, "include", "cdvslam_hip.h")).read()
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    src = re.sub(r"typedef struct.*?\}\s*\w+;", "", src, flags=re.S)
    out = {}
    for m in re.finditer(r"\b(cdv_[a-z0-9_]+)\s*\(([^;{]*?)\)\s*;", src, flags=re.S):
        name, params = m.group(1), [p.strip() for p in m.group(2).split(",")]
        w = []
        for p in params:
            if "*" not in p or p.startswith("const "):
                continue
            pname = re.findall(r"(\w+)\s*$", p)[0]
            if pname == "stream" or pname.endswith("_host"):
                continue
            w.append(pname)
        if w:
            out[name] = w
    return out


_EXEMPT_NAMES = {"cdv_last_error", "cdv_version", "cdv_fmap_padded_elems", "cdv_graph_table_offsets", "cdv_graph_read_meta_host",
                 "cdv_ba_status", "cdv_ba_factor_ticket", "cdv_ba_test_handoff", "cdv_workspace_forget",
                 "cdv_graph_corr_order", "cdv_graph_corr_records", "cdv_stream_motion"}
_EXEMPT_PATTERNS = (r"^cdv_.*_workspace_bytes$", r"^cdv_.*_workspace_init$", r"^cdv_.*bind_.*$", r"^cdv_.*_set_.*$", r"^cdv_stream_.*$",
                    r"^cdv_.*_dyn$")


def _exempt_allowed(name):
    return name in _EXEMPT_NAMES or any(re.match(p, name) for p in _EXEMPT_PATTERNS)


def coverage_problems(audited, exempt, writers=None):
    """what is wrong with a pair of tables (empty: nothing)"""
    writers = _writers() if writers is None else writers
    bad = []
    for n in sorted(writers):
        if (n in audited) == (n in exempt):
            bad.append("%s writes device memory (%s) and is in %s" % (n, ", ".join(writers[n]),
                                                                      "both tables" if n in audited else "neither table"))
    for n in sorted(exempt):
        if not _exempt_allowed(n):
            bad.append("%s is exempt without a permitted reason" % n)
        if not exempt[n] or "\n" in exempt[n]:
            bad.append("%s: the reason is one line" % n)
    return bad


def test_header_parse_finds_the_writers():
    w = _writers()
    assert len(w) >= 40
    assert w["cdv_lie_op"] == ["z"] and "out" in w["cdv_corr_fused"] and "coords" in w["cdv_transform"]
    assert w["cdv_ba_forward"][:2] == ["poses", "patches"] and "dbg" in w["cdv_ba_forward"]
    assert "cdv_version" not in w and "cdv_graph_read_meta_host" not in w and "cdv_edges_workspace_bytes" not in w


def test_every_writing_entry_point_is_audited_or_exempt():
    from tests import test_bounds_audit as B
    assert not coverage_problems(B.AUDITED, B.EXEMPT), "\n".join(coverage_problems(B.AUDITED, B.EXEMPT))
    for name, test in B.AUDITED.items():      # the test a row names exists
        assert callable(getattr(B, test, None)), (name, test)
    from cdv_slam_amd import _lib
    assert set(B.AUDITED) | set(B.EXEMPT) <= set(_lib.SIGNATURES)


def test_coverage_table_is_a_condition():
    """removing an audit without a permitted reason fails; so does an exemption that is not on the list"""
    from tests import test_bounds_audit as B
    aud = dict(B.AUDITED)
    aud.pop("cdv_lie_op")
    assert any("cdv_lie_op" in p and "neither" in p for p in coverage_problems(aud, B.EXEMPT))
    ex = dict(B.EXEMPT, cdv_lie_op="too simple to go wrong")
    assert any("cdv_lie_op is exempt without a permitted reason" in p for p in coverage_problems(aud, ex))
    assert any("both" in p for p in coverage_problems(B.AUDITED, dict(B.EXEMPT, cdv_corr_fused="x")))


def test_prologue_table_refuses_pointers_its_vector_accesses_cannot_take():
    """Alignment is judged by reading: the table prologue stores coords and loads an intrinsics row 16 bytes at a time
    (csrc/graph.hip), the header says so, and the entry point returns CDV_ERR_ARG before anything is enqueued.  The addresses
    here are never dereferenced."""
    from cdv_slam_amd import _lib
    lib = _lib.load()
    a = 0x10000

    def call(coords, intrinsics):
        return lib.cdv_update_prologue_table(a, a, a, 0, 8, 8, 8, None, None, 0, 0, 0, a, a, intrinsics, a, a, a, 4, coords, None, 0, 4, 4,
                                             4, None, None, None)
    assert call(a + 8, a) == -2 and b"coords must be 16-byte aligned" in lib.cdv_last_error()
    assert call(a, a + 4) == -2 and b"intrinsics must be 16-byte aligned" in lib.cdv_last_error()


def test_a_copy_from_one_guard_into_another_is_seen():
    """a converter that handles one element too many reads its input's guard and writes it into its output's guard: the two
    guards hold different payloads, so the copy changes bytes"""
    a = GA.Arena("cpu", "A", 0, 1 << 16)
    src, dst = a.tensor("src", np.ones(9, np.float16)), a.tensor("dst", (9,), torch.float16)
    (s0, s1), (d0, d1) = a.span("src"), a.span("dst")
    a.buf[d0:d1 + 2] = a.buf[s0:s1 + 2].clone()
    assert a.first_difference()[:3] == ("dst", "back", 1)


def test_every_alignment_the_header_states_is_checked_before_anything_is_enqueued():
    """include/cdvslam_hip.h "Alignment": a pointer that a kernel accesses through a wider vector type than its element and
    that comes with less alignment is refused with CDV_ERR_ARG.  Made-up addresses, never dereferenced: every check sits in
    front of the first launch and of any look into a workspace."""
    import ctypes
    from cdv_slam_amd import _lib
    lib = _lib.load()
    a = 0x10000
    ring = _lib.ShadowRing()
    ring.src_nchw, ring.dst_nhwc, ring.ws, ring.N, ring.C, ring.H, ring.W, ring.parity = a, a + 8, a, 1, 8, 4, 4, 0
    rp = ctypes.cast(ctypes.pointer(ring), ctypes.c_void_p)
    calls = [
        ("dst_nhwc", lambda: lib.cdv_fmap_to_nhwc(a, a + 8, 1, 8, 4, 4, 0, 1, None)),
        ("dst_nhwc", lambda: lib.cdv_fmap_sync_nhwc(a, a + 8, 1, 8, 4, 4, a, 0, None)),
        ("src_nchw", lambda: lib.cdv_fmap_sync_nhwc(a + 2, a, 1, 8, 4, 4, a, 0, None)),
        ("ws", lambda: lib.cdv_fmap_sync_nhwc(a, a, 1, 8, 4, 4, a + 8, 0, None)),
        ("dst_nhwc", lambda: lib.cdv_shadows_sync(rp, 1, None, None, 0, 8, None)),
        ("gmap_pm", lambda: lib.cdv_shadows_sync(None, 0, a, a + 8, 1, 8, None)),
        ("fmap1_nhwc", lambda: lib.cdv_fmap_ingest(a, a + 8, a, None, None, 0, 8, 4, 4, None)),
        ("fmap2_nhwc", lambda: lib.cdv_fmap_ingest(a, a, a + 8, None, None, 0, 8, 4, 4, None)),
        ("gmap_pm", lambda: lib.cdv_frame_ingest(a, a, a, None, None, 0, 8, 4, 4, a, a + 8, 1, 0, 1, None)),
        ("gmap_pm", lambda: lib.cdv_gmap_to_pixel_major(a, a + 8, 1, 8, 0, 1, None)),
        ("fmap0_nhwc", lambda: lib.cdv_corr_fused(a, a + 8, a, a, a, a, None, a, 1, 1, 1, 8, 4, 4, 1, 1, 1.0, 4.0, 2, 0, 0, 0, None)),
        ("fmap1_nhwc", lambda: lib.cdv_corr_fused(a, a, a + 8, a, a, a, None, a, 1, 1, 1, 8, 4, 4, 1, 1, 1.0, 4.0, 2, 0, 0, 0, None)),
        ("out", lambda: lib.cdv_corr_fused(a, a, a, a, a, a, None, a + 2, 1, 1, 1, 8, 4, 4, 1, 1, 1.0, 4.0, 2, 0, 0, 0, None)),
        ("pixel-major gmap", lambda: lib.cdv_corr_fused(a + 8, a, a, a, a, a, None, a, 1, 1, 1, 8, 4, 4, 1, 1, 1.0, 4.0, 2, 0, 0, 1, None)),
        ("fmap0_nhwc", lambda: lib.cdv_corr_fused_stream(a, a + 8, a, a, a, 1, 1, 1, 8, 4, 4, 1, 1, 1.0, 4.0, 1, None)),
        ("out", lambda: lib.cdv_corr_level_checked_interleaved(a, a, a, a, 0.25, a, a, a + 2, 1, 1, 1, 1, 8, 4, 4, 1.0, 0, 0, 0, None)),
        ("fmap1_nhwc", lambda: lib.cdv_update_prologue(a, a + 8, a, 0, 8, 8, 8, None, None, 0, 0, 0, a, a, a, a, a, a, 4, 1, a, None, 0, 4, 4,
                                                       None, None, None)),
        ("gmap_pm", lambda: lib.cdv_update_prologue(a, a, a, 0, 8, 8, 8, a, a + 8, 1, 0, 1, a, a, a, a, a, a, 4, 1, a, None, 0, 4, 4,
                                                    None, None, None)),
        ("fmap2_nhwc", lambda: lib.cdv_update_prologue_table(a, a, a + 8, 0, 8, 8, 8, None, None, 0, 0, 0, a, a, a, a, a, a, 4, a, None, 0,
                                                             4, 4, 4, None, None, None)),
        ("target", lambda: lib.cdv_ba_forward(a, a, a, a + 4, a, a, a, a, a, 10, 3, 0, 5, 2, None, a, 0, 10, None, None)),
        ("weight", lambda: lib.cdv_ba_forward(a, a, a, a, a + 4, a, a, a, a, 10, 3, 0, 5, 2, None, a, 0, 10, None, None)),
        ("ba_ws", lambda: lib.cdv_ba_forward(a, a, a, a, a, a, a, a, a, 10, 3, 0, 5, 2, None, a + 8, 0, 10, None, None)),
        ("coords", lambda: lib.cdv_graph_bind_corr_stream(a, a + 4, 1, 1, 1, 1, 1.0)),
        ("workspace", lambda: lib.cdv_graph_workspace_init(a + 8, 1 << 20, 16, 16, None)),
        ("workspace", lambda: lib.cdv_graph_build(a, a, 10, a + 8, 1 << 20, 16, 16, None)),
        ("workspace", lambda: lib.cdv_graph_build_table(a, a, a, 10, a + 8, 1 << 20, 16, 16, 16, None, None, None)),
        ("net", lambda: lib.cdv_edges_remove(a, 4, a, a, a, a, None, None, a + 2, 4, a, a, a, None, None, a, None, None, None, None, None,
                                             0, None, None)),
    ]
    for what, call in calls:
        rc = call()
        msg = lib.cdv_last_error().decode()
        assert rc == -2 and "aligned" in msg and what in msg, (what, rc, msg)
