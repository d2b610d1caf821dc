"""Null adj_v0 / adj_q0 at the mdg_traj_adj_small* entry points, without a GPU: the route of the wave-per-replica kernels
accepts them (a caller that wants adj_theta alone), every other route keeps refusing them.  Every call below is refused during
validation (fake pointers, nothing is launched): where the null outputs are accepted, the NEXT check answers."""
import ctypes


def _call(name, n_rep, null):
    from mdgrad_amd import _lib, ops
    lib = _lib.load()
    fake, B = ctypes.c_void_p(0x1000), ctypes.byref
    cell = _lib.make_cell([4.8] * 3)
    lj = ops.make_terms([ops.make_term(dict(kind=0, p=12, q=6, c=1.0), 2.5, 0, 2, None)], 2)
    prm = _lib.MdgTrajParams()
    prm.n_rep, prm.n_atoms, prm.n_frames, prm.n_chains, prm.ensemble = n_rep, 108, 5, 3, 0
    names = ["theta", "mass", "t", "v_t", "q_t", "pv_t"] + (["f_t"] if name.endswith("_ft") else [])
    names += ["g_v", "g_q", "g_pv", "adj_v0", "adj_q0", "adj_pv0", "adj_theta"]
    args = [None if n in null else fake for n in names]
    if "stale" in name:
        args += [3, 0, fake]
    elif "rdf" in name:
        args += [B(_lib.MdgRdfFuse(0x1000, 100, -1632.0, 0.75, 0.0175, 2.5, 0, 1)), fake]
    rc = getattr(lib, name)(B(prm), B(cell), B(lj), *args, None)
    return rc, lib.mdg_last_error()


def test_ring_route_accepts_null_state_outputs_and_the_other_routes_refuse_them():
    plain = ["mdg_traj_adj_small", "mdg_traj_adj_small_ft"]
    fused = ["mdg_traj_adj_small_rdf", "mdg_traj_adj_small_rdf_ft"]
    for out in ("adj_v0", "adj_q0"):
        # one replica: the one-workgroup-per-replica kernels (and the stale lists, which never take the ring)
        for name in plain:
            rc, msg = _call(name, 1, (out,))
            assert rc == -1 and b"null buffer" in msg, (name, out, msg)
        for n_rep in (1, 1024):
            rc, msg = _call("mdg_traj_adj_small_stale", n_rep, (out,))
            assert rc == -1 and b"null buffer" in msg, (n_rep, out, msg)
        # 1 024 replicas of one LJ 12-6 term: the ring route -- the null output passes, the null theta behind it is refused
        for name in plain:
            rc, msg = _call(name, 1024, (out, "theta"))
            assert rc == -1 and b"null theta" in msg, (name, out, msg)
        # the fused observable runs on the ring only: a launch the ring does not take is refused as before, null output or not
        for name in fused:
            rc, msg = _call(name, 1, (out,))
            assert rc == -1 and b"not available" in msg, (name, out, msg)
    # a required buffer next to the null outputs is still refused on the ring route
    for name in plain + fused:
        rc, msg = _call(name, 1024, ("adj_v0", "adj_q0", "mass"))
        assert rc == -1 and b"null buffer" in msg, (name, msg)
