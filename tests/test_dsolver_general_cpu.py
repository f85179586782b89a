"""The distributed factorisation of a non-symmetric K (follower pressure), host side: the invariant the device path relies on -- the blocks of K that join control
points of different ranks are symmetric -- on the gloo sharded model with the CPU oracle standing in for each rank's device compute (tests/test_distributed_cpu.py),
and the selection of the distributed solver in NonMatchingOpt.solve_K."""
import os

import numpy as np
import pytest
import torch.multiprocessing as mp

from tests.test_distributed_cpu import _OracleDevice, _free_port


def _pressure_spec():
    from goldfish_amd import geometry as G
    from tests.golden.make_golden import with_pressure_and_edge_tractions
    return with_pressure_and_edge_tractions(G.synthetic_shell(4, 4, nel=4, p=3, jitter=1))


def _k_worker(rank, world, port, q):
    import torch.distributed as dist
    os.environ["MASTER_ADDR"], os.environ["MASTER_PORT"] = "127.0.0.1", str(port)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    from goldfish_amd import _lib, geometry as G, sharding
    _lib.DeviceModel = _OracleDevice                     # the local compute of a rank; the sharding layer above it is the product's
    spec = _pressure_spec()
    th = G.random_thickness(spec)
    S = sharding.ShardedDeviceModel(spec, dist, rank, world, device=0, thickness_global=th)
    S.set_thickness(np.concatenate(th))
    S.set_u(G.smooth_displacement(spec, 0.5 * spec.h_th))
    S.assemble()
    K = S.csr(_lib.MAT_K)
    owner = np.empty(S.total_cp, np.int64)
    for r, own in enumerate(S.shard.owned_by_rank):
        for g in own:
            owner[S.shard.cp_off_global[g]:S.shard.cp_off_global[g + 1]] = r
    if rank == 0:
        q.put((K, owner, th))
    dist.barrier()
    dist.destroy_process_group()


@pytest.mark.parametrize("world", [2, 3])
def test_blocks_between_ranks_are_symmetric_under_a_follower_pressure(oracle_lib, world):
    """gfs_set_general on a rank's handle reads the block of a pair whose partner row is a ghost from the owned row alone (fact_value): exact only if
    K_ab = K_ba^T whenever a and b have different owners.  Only the penalty coupling joins control points of different patches, a patch is never split between
    ranks, and the follower pressure's load stiffness stays inside a patch -- checked here on the sharded K of a pressurised 4 x 4-patch shell, which is the
    unsharded oracle's K and is not symmetric inside the patches."""
    from goldfish_amd import geometry as G
    from goldfish_amd.model import arrays_from_spec
    from oracle.oracle_py import Oracle
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    port = _free_port()
    procs = [ctx.Process(target=_k_worker, args=(r, world, port, q)) for r in range(world)]
    for p in procs:
        p.start()
    K, owner, th = q.get(timeout=600)
    for p in procs:
        p.join(timeout=120)
        assert p.exitcode == 0
    spec = _pressure_spec()
    A = arrays_from_spec(spec, th)
    O = Oracle(A, thickness=np.concatenate(th), u=G.smooth_displacement(spec, 0.5 * spec.h_th))
    K0 = O.csr(0, O.assemble()[0])
    assert abs(K - K0).max() <= 1e-12 * abs(K0).max()
    assert not A.symmetric_K and abs(K - K.T).max() > 1e-10 * abs(K).max()         # the load stiffness is there
    C = K.tocoo()
    oa, ob = owner[C.row // 3], owner[C.col // 3]
    cross = oa != ob
    assert cross.sum() > 0 and len(set(oa[cross])) == world                         # every rank has blocks towards another rank
    KT = K.T.tocsr()
    diff = np.asarray(K[C.row[cross], C.col[cross]]).ravel() - np.asarray(KT[C.row[cross], C.col[cross]]).ravel()
    inside = ~cross
    diff_in = np.asarray(K[C.row[inside], C.col[inside]]).ravel() - np.asarray(KT[C.row[inside], C.col[inside]]).ravel()
    kmax = abs(K).max()
    print("world %d: |K_ab - K_ba^T| / max|K| across ranks %.2e, inside the ranks %.2e" % (world, np.abs(diff).max() / kmax, np.abs(diff_in).max() / kmax))
    # across ranks: the penalty terms of (a, b) and (b, a) are summed in different orders -- equal to round-off; the skew part lives inside the ranks
    assert np.abs(diff).max() <= 64 * np.finfo(float).eps * kmax
    assert np.abs(diff_in).max() > 1e4 * np.abs(diff).max() + 1e-10 * kmax


def test_a_sharded_problem_with_a_follower_pressure_selects_the_distributed_factorisation(monkeypatch):
    """_use_distributed_solver no longer excludes a non-symmetric K: forced (GF_SHARDED_SOLVER=distributed) or from ND_MIN_CP control points on, and only with comm;
    solve_K then builds DistributedSolver(..., general=True) -- general=False for a symmetric K -- and "replicated" keeps the gathered factorisation."""
    import scipy.sparse as sp
    from goldfish_amd import _dsolver, _solver
    from goldfish_amd.nonmatching_opt import NonMatchingOpt
    K = sp.csr_matrix(np.array([[2.0, 1.0], [0.5, -3.0]]))
    sym = {"v": False}
    monkeypatch.setattr(NonMatchingOpt, "symmetric_K", property(lambda self: sym["v"]))
    monkeypatch.setattr(NonMatchingOpt, "dev", property(lambda self: self._dev))
    monkeypatch.setattr(NonMatchingOpt, "linear_solver", "device")

    def make(dist, world, mode, ndof=6):
        nm = NonMatchingOpt.__new__(NonMatchingOpt)
        nm._dist, nm.world, nm.sharded_solver, nm.vec_iga_dof = dist, world, mode, ndof
        return nm
    for s in (False, True):
        sym["v"] = s
        assert make(object(), 2, "distributed")._use_distributed_solver()
        assert make(object(), 2, "auto", 3 * _solver.ND_MIN_CP)._use_distributed_solver()
        assert not make(object(), 2, "auto")._use_distributed_solver()
        assert not make(object(), 2, "replicated", 3 * _solver.ND_MIN_CP)._use_distributed_solver()
        assert not make(None, 1, "distributed")._use_distributed_solver()
        assert not make(object(), 1, "distributed")._use_distributed_solver()
    built = []

    class FakeDistributed:
        method = "nd-distributed"

        def __init__(self, dev, dist, group, coords=None, general=False):
            built.append(general)
            self.D, self.small_pivot = dev, False

        def solve(self, b, transpose=False, max_refine=None):
            self.transpose, self.max_refine_arg = transpose, max_refine
            self.rel_residual = self.backward_error = 0.0
            return np.linalg.solve((K.T if transpose else K).toarray(), b)

        def close(self):
            pass
    monkeypatch.setattr(_dsolver, "DistributedSolver", FakeDistributed)

    class Dev:
        def csr(self, which):
            return K

        def _allreduce(self, arr):
            return np.asarray(arr, float)
    b = np.array([1.0, 2.0])
    for s in (False, True):
        sym["v"] = s
        nm = make(object(), 2, "distributed", 2)
        nm._dev, nm._k_version, nm._group = Dev(), 1, None
        nm.splines, nm.cp_iga = [type("S", (), {"cp_hom_flat": staticmethod(lambda: np.ones((2, 4)))})()], [np.zeros(2)] * 3
        x = nm.solve_K(b, transpose=True)
        assert built[-1] == (not s) and isinstance(nm._dsolver, FakeDistributed)
        assert nm._dsolver.transpose == (not s) and nm._dsolver.max_refine_arg is None     # general mode: the solver's own refinement budget
        assert np.allclose((K.T if not s else K) @ x, b)
