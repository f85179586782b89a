"""The distributed factorisation for a non-symmetric K (follower pressure), K^T solves and blocked right-hand sides across ranks (goldfish_amd/_dsolver.py general
mode, gfs_forward_multi_dev / gfs_backward_multi_dev): on the GPU."""
import ctypes as C
import os
import re
import socket
import time

import numpy as np
import pytest

from goldfish_amd import geometry as G
from tests.test_gpu_api import _init_ranks, _rccl_world, _rel

pytestmark = pytest.mark.gpu


def _pressure_spec(nel=10):
    from tests.golden.make_golden import with_pressure_and_edge_tractions
    return with_pressure_and_edge_tractions(G.synthetic_shell(4, 4, nel=nel, p=3, jitter=2))


def _free_port():
    s = socket.socket(); s.bind(("127.0.0.1", 0)); port = s.getsockname()[1]; s.close()
    return port


def test_partial_handle_halves_for_several_right_hand_sides_equal_the_single_ones():
    """C ABI: gfs_forward_multi_dev / gfs_backward_multi_dev on a partial handle (the subtrees below the root of a one-process model, the root's control points
    eliminated "by another handle") give, column by column, the bits of gfs_forward_dev / gfs_backward_dev -- k = 3 (one group) and k = 5 (two groups on their own
    streams) -- and gfs_get_fbnd_multi the boundary contributions of gfs_get_fbnd_packed; symmetric and general mode (with a row mask that hides no row)."""
    import torch
    from goldfish_amd import _dsolver, _lib, _nd
    from goldfish_amd.model import arrays_from_spec
    L = _dsolver._bind()
    for general in (False, True):
        spec = _pressure_spec(nel=6) if general else G.synthetic_shell(3, 3, nel=6, p=3, jitter=2)
        A = arrays_from_spec(spec)
        D = _lib.DeviceModel(A, device=0)
        D.set_thickness(np.full(A.total_cp, spec.h_th))
        D.set_u(G.smooth_displacement(spec, 0.5 * spec.h_th))
        D.assemble(_lib.ASM_K)
        D.sync()
        nb_ptr, nb = D.cp_graph()
        ncp = nb_ptr.size - 1
        coords = np.stack([A.cp_hom[f] / A.weights for f in range(3)], 1)
        sym = _nd.nested_dissection_native(nb_ptr, nb, coords, leaf=48)[0]
        root = sym.nfronts - 1
        keep = np.arange(root)                                          # everything below the root
        later = sym.elim[sym.elim_off[root]:sym.elim_off[root + 1]]
        P = _dsolver._Part(L, sym, keep, (), later, np.arange(ncp), nb_ptr, nb, D.k_values_ptr(), 0, row_ok=np.ones(ncp, bool) if general else None, general=general)
        assert L.gfs_refactor(P.h) == 0, L.gfs_last_error()
        roots = np.array([P.local[t] for t in range(root) if sym.parent[t] == root], np.int64)
        nfb = 3 * int(sum(P.nbnd[r] for r in roots))
        n = 3 * ncp
        dev = torch.device("cuda", 0)
        B = torch.from_numpy(np.random.default_rng(1).standard_normal((5, n))).to(dev)
        xr = torch.from_numpy(np.random.default_rng(2).standard_normal((5, 3 * later.size))).to(dev)
        rdofs = torch.from_numpy((3 * later[:, None] + np.arange(3)).ravel()).to(dev)
        view = lambda ptr: torch.as_tensor(type("B", (), {"__cuda_array_interface__": {"shape": (n,), "typestr": "<f8", "data": (int(ptr), False), "version": 2}})(), device=dev)
        single_x, single_f = [], []
        for j in range(5):
            bj = B[j].contiguous()
            torch.cuda.synchronize()
            assert L.gfs_forward_dev(P.h, C.c_void_p(bj.data_ptr())) == 0, L.gfs_last_error()
            f = torch.zeros(max(nfb, 1), dtype=torch.float64, device=dev)
            assert L.gfs_get_fbnd_packed(P.h, roots.size, roots.ctypes.data_as(_dsolver._i64p), C.c_void_p(f.data_ptr())) == 0
            x = view(L.gfs_x_ptr(P.h))
            x[rdofs] = xr[j]
            torch.cuda.synchronize()
            assert L.gfs_backward_dev(P.h) == 0, L.gfs_last_error()
            single_x.append(x.clone()); single_f.append(f.clone())
        for k in (3, 5):
            Bk = B[:k].contiguous()
            torch.cuda.synchronize()
            assert L.gfs_forward_multi_dev(P.h, k, C.c_void_p(Bk.data_ptr())) == 0, L.gfs_last_error()
            ld = max(nfb, 1) + 7                                        # a stride longer than the packed contributions
            F = torch.zeros(k * ld, dtype=torch.float64, device=dev)
            assert L.gfs_get_fbnd_multi(P.h, k, roots.size, roots.ctypes.data_as(_dsolver._i64p), C.c_void_p(F.data_ptr()), ld) == 0, L.gfs_last_error()
            xs = [view(L.gfs_x_ptr_multi(P.h, j)) for j in range(k)]
            for j in range(k):
                xs[j][rdofs] = xr[j]
            torch.cuda.synchronize()
            assert L.gfs_backward_multi_dev(P.h, k) == 0, L.gfs_last_error()
            for j in range(k):
                assert torch.equal(F[j * ld:j * ld + max(nfb, 1)], single_f[j]), (general, k, j)
                assert torch.equal(xs[j], single_x[j]), (general, k, j)
        assert L.gfs_forward_multi_dev(P.h, 9, C.c_void_p(B.data_ptr())) != 0 and b"right-hand sides" in L.gfs_last_error()
        lib = _dsolver.lib()
        lib.gfs_destroy(P.h)
        D.close()


def _general_worker(rank, world, port, q, backend, models):
    import warnings
    import torch.distributed as dist
    from goldfish_amd.nonmatching_opt import NonMatchingOpt
    dev = _init_ranks(rank, world, port, backend)
    out = {}
    with warnings.catch_warnings(record=True) as wl:
        warnings.simplefilter("always")
        for name in models:
            spec = _pressure_spec() if name == "pressure" else G.synthetic_shell(4, 4, nel=10, p=3, jitter=2)
            nm = NonMatchingOpt.from_spec(spec, comm=dist, device=dev)
            nm.sharded_solver = "distributed"
            nm.update_uIGA(G.smooth_displacement(spec, 0.5 * spec.h_th))
            nm._assemble(3)
            B = np.random.default_rng(4).standard_normal((10, nm.vec_iga_dof))
            r = dict(symmetric=nm.symmetric_K)
            for tr in (False, True):
                t0 = time.perf_counter()
                x = nm.solve_K(B[0], transpose=tr)
                ds = nm._dsolver
                r["x", tr], r["t", tr], r["steps", tr], r["be", tr] = x, time.perf_counter() - t0, ds.refinement_steps, ds.backward_error
            r["method"], r["general"] = ds.method, ds.general
            for tr in (False, True):
                r["single", tr] = np.stack([nm.solve_K(b, transpose=tr) for b in B])
                r["X3", tr] = nm.solve_K(B[:3], transpose=tr)
                r["X10", tr] = nm.solve_K(B, transpose=tr)
            nm.update_uIGA(G.smooth_displacement(spec, 0.8 * spec.h_th))           # a new tangent: refactor (collective) and solve again
            nm._assemble(3)
            r["x1"], r["x1t"] = nm.solve_K(B[1]), nm.solve_K(B[1], transpose=True)
            r["K1"] = nm.dRIGAduIGA()
            r["host_lu"] = getattr(nm, "_hlu", None) is not None
            r["failed"] = getattr(nm, "_dsolver_failed_version", None) is not None or getattr(nm, "_dsolver_permanent_failure", None) is not None
            r["same_dsolver"] = nm._dsolver is ds
            res = [None] * world
            dist.all_gather_object(res, (nm._dsolver.method, nm._dsolver.A is not None))
            r["ranks"] = res
            out[name] = r
    out["warnings"] = [str(w.message) for w in wl if issubclass(w.category, RuntimeWarning)]
    allw = [None] * world
    dist.all_gather_object(allw, out["warnings"])
    out["all_warnings"] = allw
    if rank == 0:
        q.put(out)
    dist.barrier()
    dist.destroy_process_group()


def _run(world, backend, models):
    import torch.multiprocessing as mp
    port = _free_port()
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    procs = [ctx.Process(target=_general_worker, args=(r, world, port, q, backend, models)) for r in range(world)]
    for p in procs:
        p.start()
    out = q.get(timeout=1200)
    for p in procs:
        p.join(timeout=300)
        assert p.exitcode == 0
    return out


def _check(out, world, models):
    from goldfish_amd import _solver
    from goldfish_amd.nonmatching_opt import NonMatchingOpt
    assert not any(out["all_warnings"]), out["all_warnings"]                # no solver fallback, no unconverged solve on any rank
    for name in models:
        r = out[name]
        assert r["method"] == "nd-distributed" and all(m == "nd-distributed" and has for m, has in r["ranks"]), r["ranks"]
        assert not r["failed"] and not r["host_lu"] and r["same_dsolver"]
        assert r["general"] == (name == "pressure") and r["symmetric"] == (name != "pressure")
        # blocked = single, bit for bit, for k = 3 and k = 10 (> MAX_RHS: two rounds), K and K^T
        for tr in (False, True):
            assert np.array_equal(r["X3", tr], r["single", tr][:3]), (name, tr)
            assert np.array_equal(r["X10", tr], r["single", tr]), (name, tr)
            assert np.array_equal(r["x", tr], r["single", tr][0]), (name, tr)
        # the unsharded problem in this process: K x = b and K^T x = b to the floor of the one-GPU general mode on the same K
        spec = _pressure_spec() if name == "pressure" else G.synthetic_shell(4, 4, nel=10, p=3, jitter=2)
        nm = NonMatchingOpt.from_spec(spec)
        B = np.random.default_rng(4).standard_normal((10, nm.vec_iga_dof))
        nm.update_uIGA(G.smooth_displacement(spec, 0.5 * spec.h_th)); nm._assemble(3)
        K0 = nm.dRIGAduIGA()
        w = np.concatenate([sp_.cp_hom_flat()[:, 3] for sp_ in nm.splines])
        S = _solver.DeviceSolver(nm.dev, coords=np.stack([nm.cp_iga[f] / w for f in range(3)], 1), method="nd", general=name == "pressure", leaf=128)
        t0 = time.perf_counter(); xs = S.solve(B[0]); t_one = time.perf_counter() - t0
        t0 = time.perf_counter(); xst = S.solve(B[0], transpose=True); t_one_t = time.perf_counter() - t0
        floor, floor_t = _rel(K0 @ xs, B[0]), _rel(K0.T @ xst, B[0])
        S.close()
        err, err_t = _rel(K0 @ r["x", False], B[0]), _rel(K0.T @ r["x", True], B[0])
        print("%s, world %d: |K x - b| / |b| %.2e (one GPU %.2e), |K^T x - b| / |b| %.2e (one GPU %.2e); refinement steps %d / %d; backward errors %.1e / %.1e; "
              "solve_K %.3f / %.3f s (one process %.3f / %.3f s)" % (name, world, err, floor, err_t, floor_t, r["steps", False], r["steps", True], r["be", False], r["be", True],
                                                                    r["t", False], r["t", True], t_one, t_one_t))
        assert err < 10 * floor + 1e-12 and err_t < 10 * floor_t + 1e-12, (err, floor, err_t, floor_t)
        assert r["be", False] < 1e-12 and r["be", True] < 1e-12
        assert 0 <= r["steps", False] < 40 and 0 <= r["steps", True] < 40               # stopped by the rule, not by the budget
        if name == "pressure":
            assert r["steps", False] >= 1 and _rel(K0 @ r["x", True], B[0]) > 1e-6      # the transposed system, not the plain one
        for tr in (False, True):
            for k in (3, 9):
                assert _rel((K0.T if tr else K0) @ r["X10", tr][k], B[k]) < 10 * (floor_t if tr else floor) + 1e-10, (name, tr, k)
        nm.update_uIGA(G.smooth_displacement(spec, 0.8 * spec.h_th)); nm._assemble(3)
        K1 = nm.dRIGAduIGA()
        assert abs(K1 - r["K1"]).max() < 1e-9 * abs(K1).max()
        assert _rel(K1 @ r["x1"], B[1]) < 1e-7 and _rel(K1.T @ r["x1t"], B[1]) < 1e-7


@pytest.mark.parametrize("world", [2, 3])
def test_distributed_general_mode_on_a_sharded_pressure_model(world):
    """A sharded 4 x 4-patch shell with a follower pressure on every second patch, GF_SHARDED_SOLVER=distributed, world 2 and 3 over gloo on the one GPU: solve_K(b)
    and solve_K(b, transpose=True) take the distributed factorisation of the symmetric part on every rank (no fallback, no host LU), reach the one-GPU general mode's
    floor for K and K^T of the unsharded model, report a bounded number of refinement steps; k = 3 and k = 10 right-hand sides equal the single solves bit for bit
    (the pressure model and a symmetric one); a new assembly is refactored and solved."""
    _check(_run(world, "gloo", ("pressure", "symmetric")), world, ("pressure", "symmetric"))


def test_distributed_general_mode_over_rccl():
    """The same over RCCL (one GPU per rank, or two ranks sharing the GPU of a one-GPU box): the boundary contributions of k columns by one all_gather_into_tensor
    per level, the K^T products by one all-reduce of device tensors."""
    world, backend = _rccl_world(3)
    _check(_run(world, backend, ("pressure",)), world, ("pressure",))


def test_tube_example_under_torchrun_on_two_ranks():
    """examples/tube_shape_opt.py launched as the reference launches its demos under MPI: ``python -m torch.distributed.run --nproc-per-node 2`` on one GPU, the
    distributed factorisation forced (GF_SHARDED_SOLVER=distributed): the non-symmetric K and its K^T adjoint solves across the ranks, no solver fallback, and the
    optimum of the one-process run."""
    import importlib.util, subprocess, sys
    here = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    env = dict(os.environ, GF_SHARDED_SOLVER="distributed", HSA_ENABLE_IPC_MODE_LEGACY="0")
    out = subprocess.run([sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", "2", "--master-addr", "127.0.0.1", "--master-port", str(_free_port()),
                          os.path.join(here, "examples", "tube_shape_opt.py")], env=env, capture_output=True, text=True, timeout=1500)
    text = out.stdout + out.stderr
    assert out.returncode == 0, out.stdout[-2000:] + out.stderr[-2000:]
    assert "falling back" not in text and "cannot be used for this model" not in text, text[-2000:]
    m = re.findall(r"final internal energy\s+([0-9.eE+-]+), radius standard deviation\s+([0-9.eE+-]+)", out.stdout)
    assert len(m) == 1, out.stdout[-2000:]
    w1, s1 = float(m[0][0]), float(m[0][1])
    spec_ = importlib.util.spec_from_file_location("tube_shape_opt", os.path.join(here, "examples", "tube_shape_opt.py"))
    mod = importlib.util.module_from_spec(spec_)
    spec_.loader.exec_module(mod)
    ref = mod.run(verbose=False)
    print("tube: two ranks W %.9e, std %.9e; one process W %.9e, std %.9e" % (w1, s1, ref["w1"], ref["r1"][0]))
    assert abs(w1 / ref["w1"] - 1.0) < 2e-4 and abs(s1 - ref["r1"][0]) < 2e-6, (w1, ref["w1"], s1, ref["r1"][0])
