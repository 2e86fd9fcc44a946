"""GPU, world_size 2: Evaluator's per-sample path under data parallel, two processes sharing the one GPU of the test box over the
`gloo` backend (as tests/test_dist_gpu.py starts them).  Each rank evaluates its half of the batch and counts its own rows: no
all-gather; result() and per_class() sum a copy of the counters over the ranks and must equal the single-process values."""
import os

import numpy as np
import pytest
import torch
import torch.multiprocessing as mp

pytestmark = pytest.mark.gpu

import eval_model as E  # noqa: E402
from test_dist_gpu import _free_port  # noqa: E402
from test_eval_head_gpu import ALPHAS3, StubModal3, dev  # noqa: E402

WORLD = 2
CASE = (3, 64, 4)


def _worker(rank, port, outdir):
    import torch.distributed as dist
    os.environ["MASTER_ADDR"], os.environ["MASTER_PORT"] = "127.0.0.1", str(port)
    dist.init_process_group("gloo", rank=rank, world_size=WORLD)
    torch.cuda.set_device(0)
    from mla_hip import Comm, Evaluator
    gathers = []
    gather_rows = Comm.allgather_rows
    Comm.allgather_rows = lambda self, t: (gathers.append(tuple(t.shape)), gather_rows(self, t))[1]
    M, B, C = CASE
    outs, label = E.sample_dense_case(M, B, C)
    per = B // WORLD
    sl = slice(rank * per, (rank + 1) * per)
    comm = Comm()
    assert comm.active and comm.world == WORLD
    ev = Evaluator(StubModal3(C), dynamic=True, dynamic_mode="sample", comm=comm)
    ev.update(*[dev(o[sl]) for o in outs], dev(label[sl], torch.int64))
    result, per_class = ev.result(), ev.per_class()
    torch.cuda.synchronize()
    torch.save({"result": torch.tensor(result, dtype=torch.float64), "per_class": torch.from_numpy(per_class),
                "local": ev.counts.cpu().view(2 + M, C).long(), "gathers": torch.tensor(len(gathers))},
               os.path.join(outdir, f"ev{rank}.pt"))
    dist.barrier()
    dist.destroy_process_group()


@pytest.mark.timeout(300)
def test_two_rank_sample_eval_equals_single_process_without_all_gather(tmp_path):
    from mla_hip import Evaluator
    M, B, C = CASE
    ctx = mp.get_context("spawn")
    port = _free_port()
    procs = [ctx.Process(target=_worker, args=(r, port, str(tmp_path))) for r in range(WORLD)]
    for p in procs:
        p.start()
    try:
        for p in procs:
            p.join(timeout=200)
            assert p.exitcode == 0
    finally:
        for p in procs:                                     # a rank that outlived its time limit is not left behind
            if p.is_alive():
                p.kill()
    outs, label = E.sample_dense_case(M, B, C)
    ev = Evaluator(StubModal3(C), dynamic=True, dynamic_mode="sample")
    ev.update(*[dev(o) for o in outs], dev(label, torch.int64))
    want = ev.per_class()
    assert (want == E.eval_rows(outs, label, 1, ALPHAS3).counts).all()
    ranks = [torch.load(tmp_path / f"ev{r}.pt", weights_only=True) for r in range(WORLD)]
    for r in ranks:
        assert (r["per_class"].numpy() == want).all()
        assert tuple(r["result"].tolist()) == ev.result()
        assert int(r["gathers"]) == 0                                   # each rank counted its own rows: nothing was gathered
        assert int(r["local"][0].sum()) == B // WORLD                   # the local counters stay local
    assert ((ranks[0]["local"] + ranks[1]["local"]).numpy() == want).all()
    assert isinstance(want, np.ndarray)
