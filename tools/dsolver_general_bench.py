"""Times of the distributed factorisation in general mode (a follower pressure's non-symmetric K): solve_K and solve_K(transpose=True) with their refinement
steps, and k = 3 right-hand sides in one blocked call against three single calls -- two ranks sharing GPU 0 over RCCL (socket transport, as the one-GPU tests run),
next to the one-process general mode (DeviceSolver(general=True)) on the same K.  Models: the sharded tube of examples/tube_shape_opt.py and a quarter of C4
(8 x 8 patches, nel 48) with a follower pressure on every second patch.

    python tools/dsolver_general_bench.py [tube|c4q ...]
"""
import os
import socket
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def _spec(name):
    from goldfish_amd import geometry as G
    if name == "tube":
        return G.pressurised_tube(E=1.0e12, pressure=1.0, shape=lambda th: 1.0 + 0.03 * (1.0 - np.cos(4.0 * th)))
    spec = G.synthetic_shell(8, 8, nel=48, p=3, jitter=2)
    spec.pressure = [(-1.0e4 if s % 2 == 0 else 0.0) * (1 + s % 4) for s in range(len(spec.patches))]
    return spec


def _state(nm, spec, name):
    from goldfish_amd import geometry as G
    if name == "tube":
        nm.solve_nonlinear_nonmatching_problem(rtol=1e-9, max_it=30)
    else:
        nm.update_uIGA(G.smooth_displacement(spec, 0.5 * spec.h_th))
    nm._assemble(3)


def _timed(f, reps=3):
    f()
    t = []
    for _ in range(reps):
        t0 = time.perf_counter()
        f()
        t.append(time.perf_counter() - t0)
    return float(np.median(t))


def _worker(rank, world, port, name, q):
    import torch
    import torch.distributed as dist
    os.environ["MASTER_ADDR"], os.environ["MASTER_PORT"] = "127.0.0.1", str(port)
    os.environ.update(NCCL_HOSTID="goldfish-bench-rank-%d" % rank, NCCL_SOCKET_IFNAME="lo", NCCL_IB_DISABLE="1")
    torch.cuda.set_device(0)
    dist.init_process_group("nccl", rank=rank, world_size=world, device_id=torch.device("cuda", 0))
    from goldfish_amd.nonmatching_opt import NonMatchingOpt
    spec = _spec(name)
    nm = NonMatchingOpt.from_spec(spec, comm=dist, device=0)
    nm.sharded_solver = "distributed"
    _state(nm, spec, name)
    B = np.random.default_rng(3).standard_normal((3, nm.vec_iga_dof))
    out = {}
    for tr in (False, True):
        out["t_solve", tr] = _timed(lambda: nm.solve_K(B[0], transpose=tr))
        out["steps", tr] = nm._dsolver.refinement_steps
    out["t_multi3"] = _timed(lambda: nm.solve_K(B, transpose=True))
    out["t_single3"] = _timed(lambda: [nm.solve_K(b, transpose=True) for b in B])
    out["method"], out["ndof"] = nm._dsolver.method, nm.vec_iga_dof
    if rank == 0:
        q.put(out)
    dist.barrier()
    dist.destroy_process_group()


def main(names):
    import torch.multiprocessing as mp
    from goldfish_amd import _solver
    from goldfish_amd.nonmatching_opt import NonMatchingOpt
    for name in names:
        s = socket.socket(); s.bind(("127.0.0.1", 0)); port = s.getsockname()[1]; s.close()
        ctx = mp.get_context("spawn")
        q = ctx.Queue()
        procs = [ctx.Process(target=_worker, args=(r, 2, port, name, q)) for r in range(2)]
        for p in procs:
            p.start()
        d = q.get(timeout=3000)
        for p in procs:
            p.join(timeout=600)
        spec = _spec(name)
        nm = NonMatchingOpt.from_spec(spec)
        _state(nm, spec, name)
        w = np.concatenate([sp_.cp_hom_flat()[:, 3] for sp_ in nm.splines])
        S = _solver.DeviceSolver(nm.dev, coords=np.stack([nm.cp_iga[f] / w for f in range(3)], 1), method="nd", general=True)
        B = np.random.default_rng(3).standard_normal((3, nm.vec_iga_dof))
        t1 = {tr: _timed(lambda: S.solve(B[0], transpose=tr)) for tr in (False, True)}
        t1m = _timed(lambda: S.solve_multi(B, transpose=True))
        S.close()
        print("%s (%d dofs, %s): two ranks on one GPU: solve_K %.4f s (%d refinement steps), transposed %.4f s (%d steps); k = 3 blocked %.4f s against 3 single %.4f s"
              " | one process, general mode: solve %.4f s, transposed %.4f s, k = 3 %.4f s"
              % (name, d["ndof"], d["method"], d["t_solve", False], d["steps", False], d["t_solve", True], d["steps", True], d["t_multi3"], d["t_single3"],
                 t1[False], t1[True], t1m), flush=True)


if __name__ == "__main__":
    main(sys.argv[1:] or ["tube", "c4q"])
