"""GPU, world_size 2: the data-parallel JointTrainer (mla_hip/joint.py + dist.py), two processes sharing the one GPU of the
test box over `gloo` (RCCL refuses two ranks on one device), each with half the batch, against ONE process running the
whole batch.  Exercised: the packed (dW|db|losses) all-reduce, inv_batch = 1/(B*world), each encoder's gradient all-reduce,
the OGM coefficients from the all-gathered global-batch half-head logits, and the modulation after the all-reduce.

Transformer classifiers (no BatchNorm: LayerNorm is per token), so sharding the batch is exactly the global-batch step up to
summation order.  Modal3 under OGM: its CAV-MAE audio encoder has a 4-D patch-embedding gradient, so the modulation really
scales something; a coefficient taken from the local half batch would differ from the global one."""
import os

import pytest
import torch
import torch.multiprocessing as mp

pytestmark = pytest.mark.gpu

from oracle import mla_oracle as O  # noqa: E402
from test_dist_gpu import T_DEPTH, T_VOCAB, WORLD, _free_port, _transformer_case  # noqa: E402
from util import assert_close, assert_close_robust  # noqa: E402


def _build(which, modulation, comm=None):
    import mla_hip
    A0, sd, inputs, label = _transformer_case(which)
    M = 2 if which == "m3ae" else 3
    C = sd["fusion_module.fc_out.weight"].shape[0]
    sd.update({f"fusion_module.fc_out.{k}": v for k, v in O.make_head_params(768 * M, C, 977).items()})

    class A(A0):
        gs_flag = False
    A.modulation = modulation
    cls = mla_hip.M3AEClassifier if which == "m3ae" else mla_hip.Modal3Classifier
    model = cls(A(), depth=T_DEPTH, text_vocab_size=T_VOCAB, seed=0)
    model.load_state_dict(sd)
    tr = mla_hip.JointTrainer(model, lr=1e-3, momentum=0.9, weight_decay=1e-4, modulation=modulation, alpha=0.3, comm=comm)
    return model, tr, inputs, label


def _run(model, tr, inputs, label, sl):
    out = {}
    for s in range(2):
        losses = tr.train_step(*[x[sl].cuda() for x in inputs], label[sl].cuda(), s)
        torch.cuda.synchronize()
        out[f"s{s}.losses"] = {k: v.cpu().clone() for k, v in losses.items()}
        if "coeff" in tr.last:
            out[f"s{s}.coeff"] = tr.last["coeff"].cpu().clone()
    out["state"] = {k: v.cpu().clone() for k, v in model.state_dict().items()}
    return out


def _worker(rank, port, outdir, which, modulation):
    import torch.distributed as dist
    os.environ["MASTER_ADDR"], os.environ["MASTER_PORT"] = "127.0.0.1", str(port)
    dist.init_process_group("gloo", rank=rank, world_size=WORLD)
    torch.cuda.set_device(0)
    from mla_hip import Comm
    comm = Comm(bucket_bytes=1 << 20)
    assert comm.active and comm.world == WORLD
    model, tr, inputs, label = _build(which, modulation, comm)
    per = label.shape[0] // WORLD
    res = _run(model, tr, inputs, label, slice(rank * per, (rank + 1) * per))
    torch.save(res, os.path.join(outdir, f"rank{rank}.pt"))
    dist.barrier()
    dist.destroy_process_group()


@pytest.mark.timeout(900)
@pytest.mark.parametrize("which,modulation", [("m3ae", "Normal"), ("m3ae", "OGM"), ("modal3", "Normal"), ("modal3", "OGM")])
def test_two_rank_joint_trainer_equals_global_batch(tmp_path, which, modulation):
    ctx = mp.get_context("spawn")
    port = _free_port()
    procs = [ctx.Process(target=_worker, args=(r, port, str(tmp_path), which, modulation)) for r in range(WORLD)]
    for p in procs:
        p.start()
    for p in procs:
        p.join(timeout=600)
        assert p.exitcode == 0
    r0 = torch.load(tmp_path / "rank0.pt", weights_only=True)
    r1 = torch.load(tmp_path / "rank1.pt", weights_only=True)
    model, tr, inputs, label = _build(which, modulation)
    one = _run(model, tr, inputs, label, slice(0, label.shape[0]))
    for s in range(2):
        for k, v in one[f"s{s}.losses"].items():
            assert_close(r0[f"s{s}.losses"][k], v, atol=1e-5, name=f"s{s} global {k}")
            assert torch.equal(r0[f"s{s}.losses"][k], r1[f"s{s}.losses"][k]), f"ranks must report the same {k}"
        if modulation != "Normal":
            assert_close(r0[f"s{s}.coeff"], one[f"s{s}.coeff"], atol=1e-6, name=f"s{s} coefficients (global batch)")
            assert torch.equal(r0[f"s{s}.coeff"], r1[f"s{s}.coeff"])
    for k, v in one["state"].items():
        if v.dtype != torch.float32:
            continue
        assert torch.equal(r0["state"][k], r1["state"][k]), f"ranks must hold identical {k}"
        if k.startswith("fusion_module"):
            assert_close(r0["state"][k], v, atol=1e-5, name=k)
        else:
            assert_close_robust(r0["state"][k], v, rel_l2=1e-5, elem_tol=1e-5, frac=0.999, name=k)
