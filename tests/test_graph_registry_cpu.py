"""The index registry's answer for a workspace address that holds no index (no GPU: every call below returns from its
argument checks, before anything touches a device)."""
import ctypes


def test_an_address_with_only_a_bound_corr_stream_holds_no_index():
    """cdv_graph_bind_corr_stream on an address the library has never built or initialised an index in makes a registry
    entry without a layout.  Every reader must treat it as "no built graph": the two pointer getters return NULL (not the
    workspace base, which an all-zero layout would give) and the others their usual error."""
    from cdv_slam_amd import _lib
    lib = _lib.load()
    ws = ctypes.c_void_p(0x7f0000001000)   # never dereferenced
    lib.cdv_workspace_forget(ws)
    try:
        assert lib.cdv_graph_bind_corr_stream(ws, None, 4, 4, 4, 4, 1.0) == 0
        assert lib.cdv_graph_corr_order(ws) is None
        assert lib.cdv_graph_corr_records(ws) is None
        out = (ctypes.c_int64 * 8)()
        for rc in (lib.cdv_graph_read_meta_host(ws, out, None), lib.cdv_graph_get_unique(ws, None, 0, None, 4, None),
                   lib.cdv_neighbors(ws, 4, None, None, None)):
            assert rc == -2 and b"no built graph" in lib.cdv_last_error()
        rc = lib.cdv_ba_forward(None, None, None, None, None, None, None, None, None, 10, 3, 0, 4, 2, ws, None, 0, 10, None, None)
        assert rc == -2 and b"graph_ws has no built graph" in lib.cdv_last_error()
        dyn = (ctypes.c_int32 * 8)()
        rc = lib.cdv_ba_forward_dyn(None, None, None, None, None, None, None, None, None, 10, 3, 4, dyn, 2, ws, None, 0, 10, None)
        assert rc == -4 and b"patch table" in lib.cdv_last_error()
    finally:
        lib.cdv_workspace_forget(ws)
