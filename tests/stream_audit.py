"""TEST INFRASTRUCTURE: a per-update audit of the device-resident frame stream (cdv_slam_amd.stream.DeviceStreamRunner).

The closed-loop tests compare edge lists, keyframe counts, the trajectory and the median depth with the oracle runner; the
operator stub reads correlation channels 0-3 only.  This audit looks at everything one update produced and every ring it
read, frame by frame:

  a. lists      the update-time edge lists equal the oracle runner's (StreamOracle.last), bit for bit
  b. rings      fmap1 interior bit-exact, fmap2 interior and the planar tiles within one f16 ulp, the ring margins zero,
                gmap_pm == the pixel-major permutation of gmap (bit for bit) -- after every frame, dropped ones included
                (this is what checks the keyframe shift of each buffer)
  c. corr       on frames that kept their keyframe (the rings after the frame are the rings the update read): corr_out[0, :E]
                against the float64 O.slam_corr at the runner's own coordinates and ring slots, overall and per level
  d. bounds     rows [E, ecap) of corr_out and coords_buf still hold the sentinel written before the frame
  e. stub       target / weight of the update equal a numpy float32 recompute from coords_buf and corr_out channels 0-3
  f. inactive   the rows pruned this frame went to target_inac / weight_inac (and ii/jj/kk_inac) bit for bit, in list order,
                and the kept rows to the other twin

Where it reads the update's state (cdv_stream_frame, csrc/stream.hip): the frame's update runs on the lists of twin `cur`, and
cdv_stream_keyframe compacts them into twin `oth` and sets cur = oth.  So after a frame, twin 1 - run.cur holds the lists as the
update saw them, with the target / weight the stub wrote; dynamic block slot - 1 holds (n, E) of the update, block `slot` the
counts after keyframe().  coords_buf[0, :E] and corr_out[0, :E] are that update's rows, in list order.

The pure checks (check_corr, compare_rings, stub_recompute, pruned_rows) take plain arrays so that tests/test_stream_audit_cpu.py
can show that each one rejects what it is meant to reject."""
import numpy as np
import torch

from oracle import oracle as O

CORR_SENTINEL = 0x7E5A            # an f16 NaN with a payload no arithmetic produces
COORDS_SENTINEL = 0x7FA5A5A5      # an f32 NaN, likewise
STUB_ULPS = 4                     # tanhf / expf against numpy's tanh / exp, plus the roundings of the stub's three operations
# f16 ulps between the device rings and the oracle's.  fmap2: the device sums each 4 x 4 block in a DPP tree, the oracle in
# window order (observed: 0 in every closed-loop run).  gmap: the tiles' bilinear blend, float32 on both sides (observed: 1)
FMAP2_ULPS = 1
GMAP_ULPS = 1


def corr_tol(truth):
    """the correlation bound of test_corr_fused_vs_oracle"""
    return 2.0 ** -8 * np.abs(truth).max() + 2.0 ** -10


def corr_errors(got, truth):
    """{part: (max |got - truth| / tol, mean |got - truth| / tol)} for all 882 channels and for each level alone (even
    channels: level 0, odd: level 1 -- SLAM.corr's stack-then-view layout), each against its own tol"""
    out = {}
    for part, sl in (("all", slice(None)), ("level0", slice(0, None, 2)), ("level1", slice(1, None, 2))):
        t = truth[:, sl]
        d = np.abs(got[:, sl].astype(np.float64) - t)
        tol = corr_tol(t)
        out[part] = (float(d.max()) / tol, float(d.mean()) / tol)
    return out


def check_corr(got, truth):
    """max error within tol and mean error within tol / 10, overall and per level; returns corr_errors"""
    assert got.shape == truth.shape and got.shape[1] == 882, (got.shape, truth.shape)
    assert np.isfinite(got).all(), "non-finite correlation (a row the launch did not write?)"
    errs = corr_errors(got, truth)
    for part, (mx, mean) in errs.items():
        assert mx <= 1.0, ("correlation max error / tol", part, mx)
        assert mean <= 0.1, ("correlation mean error / tol", part, mean)
    return errs


def f16_ulps(a, b):
    """elementwise distance of two f16 tensors in units in the last place (+0 and -0 are the same point)"""
    def ordered(x):
        i = x.contiguous().view(torch.int16).to(torch.int32)
        return torch.where(i < 0, -(i & 0x7FFF), i)
    return (ordered(a) - ordered(b)).abs()


def live_frames(n, slots):
    """the keyframes whose ring slot is live after keyframe() left n of them: the newest `slots - 1` (the slot of frame n - slots
    is the one the next frame overwrites; after a drop it holds the removed newest frame's leftover on both sides)"""
    return list(range(max(0, n - slots + 1), n))


def compare_rings(fmap1, fmap2, gmap, gmap_pm, o_fmap1, o_fmap2, o_gmap, n, M, pad):
    """device rings (padded channels-last fmap1 / fmap2, planar gmap [pmem M, C, 3, 3], pixel-major gmap_pm [pmem M, 9, C],
    torch) against the oracle's (planar numpy) over the live slots; o_* None: the device's own consistency only.  Returns the
    largest fmap2 and gmap distances in f16 ulps."""
    py, px = pad
    mem, pmem = fmap1.shape[0], gmap.shape[0] // M
    for ring in (fmap1, fmap2):        # the zero margins the correlation's unguarded window loads rely on
        assert not ring[:, :py].any() and not ring[:, -py:].any(), "ring margin (rows) not zero"
        assert not ring[:, :, :px].any() and not ring[:, :, -px:].any(), "ring margin (columns) not zero"
    fs = [f % mem for f in live_frames(n, mem)]
    ts = torch.cat([torch.arange(M) + (f % pmem) * M for f in live_frames(n, pmem)]) if n > 0 else torch.zeros(0, dtype=torch.long)
    ts = ts.to(gmap.device)
    C = gmap.shape[1]
    pm = gmap[ts].reshape(-1, C, 9).transpose(1, 2)
    assert torch.equal(gmap_pm[ts], pm), "gmap_pm is not the pixel-major permutation of gmap"
    worst = {"fmap2_ulps": 0, "gmap_ulps": 0}
    if o_fmap1 is None or not fs:
        return worst
    dev = fmap1.device
    i1 = fmap1[fs, py:-py, px:-px].permute(0, 3, 1, 2)
    assert torch.equal(i1, torch.as_tensor(o_fmap1[fs], device=dev)), "fmap1 ring differs from the oracle's"
    i2 = fmap2[fs, py:-py, px:-px].permute(0, 3, 1, 2)
    u2 = int(f16_ulps(i2, torch.as_tensor(o_fmap2[fs], device=dev)).max())
    assert u2 <= FMAP2_ULPS, ("fmap2 ring differs from the oracle's by %d ulps" % u2)
    ug = int(f16_ulps(gmap[ts], torch.as_tensor(o_gmap, device=dev)[ts]).max())
    assert ug <= GMAP_ULPS, ("gmap ring differs from the oracle's by %d ulps" % ug)
    worst.update(fmap2_ulps=u2, gmap_ulps=ug)
    return worst


def stub_recompute(coords, corr4, gain):
    """the operator stub (cdv_slam_amd/stream.py, csrc/stream.hip stream_operator_stub_kernel) in numpy float32: coords [E,2,3,3],
    corr4 [E,4] -> target [E,2], weight [E,2]"""
    c = corr4.astype(np.float32)
    g = np.float32(gain)
    target = np.stack([coords[:, 0, 1, 1] + g * np.tanh(c[:, 0]), coords[:, 1, 1, 1] + g * np.tanh(c[:, 1])], -1)
    weight = np.float32(1.0) / (np.float32(1.0) + np.exp(-c[:, 2:4]))
    return target.astype(np.float32), weight.astype(np.float32)


def ulps32(got, want):
    """largest |got - want| in float32 ulps of want"""
    if got.size == 0:
        return 0.0
    return float((np.abs(got.astype(np.float64) - want) / np.spacing(np.abs(want).astype(np.float32))).max())


def pruned_rows(ii, jj, kk, n, M, ki, rw, dropped):
    """keyframe() on update-time lists (slam.py:415-458, oracle/edges_py.py): (indices of the rows pruned to the inactive
    lists, indices of the rows kept, ii, jj, kk after the index shift of a drop)"""
    keep = np.ones(len(ii), bool)
    if dropped:
        k = n - ki
        keep = (ii != k) & (jj != k)
        kk = np.where(ii > k, kk - M, kk)
        jj = np.where(jj > k, jj - 1, jj)
        ii = np.where(ii > k, ii - 1, ii)
        n -= 1
    old = keep & (kk // M < n - rw)
    return np.nonzero(old)[0], np.nonzero(keep & ~old)[0], ii, jj, kk


class StreamAudit:
    """Call arm(run) before a frame to audit it, then audit(run, ...) after it; as closed_loop's `audit` hook it does both (it
    audits frame f and arms frame f + 1).  corr_every: the correlation (c) on every k-th kept frame; rings (b) every frame."""

    def __init__(self, name, corr_every=1):
        self.name, self.corr_every = name, corr_every
        self.armed = None
        self.kept = 0
        self.worst = {"corr": 0.0, "corr_level0": 0.0, "corr_level1": 0.0, "corr_mean": 0.0, "fmap2_ulps": 0, "gmap_ulps": 0,
                      "stub_target_ulps": 0.0, "stub_weight_ulps": 0.0}
        self.counts = {"frames": 0, "corr": 0, "bounds": 0, "inactive": 0, "pruned_rows": 0}

    def arm(self, run):
        """write the sentinels over every row of corr_out / coords_buf; note the inactive count"""
        run.corr_out.view(torch.int16).fill_(CORR_SENTINEL)
        run.coords_buf.view(torch.int32).fill_(COORDS_SENTINEL)
        self.armed = int(run.dyn[run.slot, 2].item())      # CDV_DYN_EINAC before the frame

    def __call__(self, f, run, so, dropped):
        self.audit(run, so, dropped)
        self.arm(run)

    def audit(self, run, so=None, dropped=None):
        from cdv_slam_amd import ops
        ring = getattr(run, "_desc", None)
        ring = (ring.ring_blocks or 8) if ring is not None else 8
        blk_u, blk_k = run.dyn[(run.slot - 1) % ring].cpu().numpy(), run.dyn[run.slot].cpu().numpy()
        assert blk_k[7] == 0, "capacity error on the device"
        n_after = int(blk_k[0])
        self.counts["frames"] += 1
        w = compare_rings(run.fmap1, run.fmap2, run.gmap, run.gmap_pm, None if so is None else so.fmap1,
                          None if so is None else so.fmap2, None if so is None else so.gmap, n_after, run.M,
                          (ops.FMAP_PADY, ops.FMAP_PADX))
        for k, v in w.items():
            self.worst[k] = max(self.worst[k], v)
        if run.frames < 8:     # before initialisation only the rings are filled
            self.armed = None
            return
        n, E = int(blk_u[0]), int(blk_u[1])
        drop_dev = n_after == n - 1
        assert n_after in (n, n - 1)
        if dropped is not None:
            assert bool(dropped) == drop_dev, (dropped, n, n_after)
        o = 1 - run.cur
        ii, jj, kk = (t[o, :E].cpu().numpy() for t in (run._ii, run._jj, run._kk))
        target, weight = run._target[o, :E].cpu().numpy(), run._weight[o, :E].cpu().numpy()
        # (a) the lists the update ran on
        if so is not None:
            assert len(so.last["ii"]) == E, (len(so.last["ii"]), E)
            assert (np.array_equal(ii, so.last["ii"]) and np.array_equal(jj, so.last["jj"])
                    and np.array_equal(kk, so.last["kk"])), "update-time edge lists differ from the oracle runner's"
        coords = run.coords_buf[0, :E].cpu().numpy()
        corr = run.corr_out[0, :E]
        # (d) nothing written past the list
        if self.armed is not None:
            assert bool((run.corr_out[0, E:].view(torch.int16) == CORR_SENTINEL).all()), "corr_out written past row E"
            assert bool((run.coords_buf[0, E:].view(torch.int32) == COORDS_SENTINEL).all()), "coords_buf written past row E"
            self.counts["bounds"] += 1
        # (e) the operator stub
        t_want, w_want = stub_recompute(coords, corr[:, :4].float().cpu().numpy(), run.gain)
        ut, uw = ulps32(target, t_want), ulps32(weight, w_want)
        assert ut <= STUB_ULPS and uw <= STUB_ULPS, ("stub", ut, uw)
        self.worst["stub_target_ulps"] = max(self.worst["stub_target_ulps"], ut)
        self.worst["stub_weight_ulps"] = max(self.worst["stub_weight_ulps"], uw)
        # (f) the pruned rows -> the inactive lists, the kept ones -> the other twin
        old, kept, ii2, jj2, kk2 = pruned_rows(ii, jj, kk, n, run.M, run.ki, run.rw, drop_dev)
        E_after, Ei = int(blk_k[1]), int(blk_k[2])
        assert E_after == len(kept), (E_after, len(kept))
        c = run.cur
        for name, got, want in (("ii", run._ii[c, :E_after], ii2[kept]), ("jj", run._jj[c, :E_after], jj2[kept]),
                                ("kk", run._kk[c, :E_after], kk2[kept]), ("target", run._target[c, :E_after], target[kept]),
                                ("weight", run._weight[c, :E_after], weight[kept])):
            assert np.array_equal(got.cpu().numpy(), want), ("kept rows", name)
        if self.armed is not None:
            a = self.armed
            assert Ei - a == len(old), (Ei - a, len(old))
            for name, got, want in (("ii", run.ii_inac, ii2[old]), ("jj", run.jj_inac, jj2[old]), ("kk", run.kk_inac, kk2[old]),
                                    ("target", run.target_inac, target[old]), ("weight", run.weight_inac, weight[old])):
                assert np.array_equal(got[a:Ei].cpu().numpy(), want), ("inactive rows", name)
            self.counts["inactive"] += 1
            self.counts["pruned_rows"] += len(old)
        self.armed = None
        # (c) the correlation, when the rings after the frame are those the update read
        if drop_dev:
            return
        self.kept += 1
        if (self.kept - 1) % self.corr_every:
            return
        self.check_corr(run, coords, corr, kk, jj)

    def check_corr(self, run, coords, corr, kk, jj):
        from cdv_slam_amd import ops
        f1 = ops.fmap_interior(run.fmap1).permute(0, 3, 1, 2).contiguous().cpu().numpy()
        f2 = ops.fmap_interior(run.fmap2).permute(0, 3, 1, 2).contiguous().cpu().numpy()
        truth = O.slam_corr(run.gmap.cpu().numpy(), f1, f2, np.ascontiguousarray(coords), kk % (run.M * run.pmem),
                            jj % run.mem, 3, "truth")
        errs = check_corr(corr.float().cpu().numpy(), truth)
        self.worst["corr"] = max(self.worst["corr"], errs["all"][0])
        self.worst["corr_level0"] = max(self.worst["corr_level0"], errs["level0"][0])
        self.worst["corr_level1"] = max(self.worst["corr_level1"], errs["level1"][0])
        self.worst["corr_mean"] = max(self.worst["corr_mean"], max(m for _, m in errs.values()))
        self.counts["corr"] += 1

    def bounds(self):
        return {"corr": 1.0, "corr_level0": 1.0, "corr_level1": 1.0, "corr_mean": 0.1, "fmap2_ulps": FMAP2_ULPS, "gmap_ulps": GMAP_ULPS,
                "stub_target_ulps": STUB_ULPS, "stub_weight_ulps": STUB_ULPS}

    def log(self, kind):
        from tests.ba_checks import _log
        print("stream audit [%s]: %s, %s" % (self.name, self.counts, {k: round(float(v), 4) for k, v in self.worst.items()}))
        _log(kind, self.name, {**self.worst, **self.counts}, self.bounds())
