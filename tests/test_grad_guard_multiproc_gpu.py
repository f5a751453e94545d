"""TrainEngine(max_grad_norm=...) over two data-parallel ranks (gloo, both on cuda:0): the norm is that of the AVERAGED gradient,
so grad_norm, the clipping coefficient and every master weight are bit-identical across the ranks, whichever half batch a rank
trained on."""
import os
import socket
import sys
import time

import pytest
import torch
import torch.multiprocessing as mp

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
STEPS = 3
WORKER_LIMIT_S = 240          # per worker: two engines x three tiny steps + the process group (torch's import is most of it)


def _free_port():
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        return s.getsockname()[1]


def _build():
    sys.path.insert(0, os.path.join(ROOT, "kindergarten-vq-vae_amd"))
    from models.shelgon3.Shelgon import Shelgon
    from models.shelgon3.VectorQuantizer import VectorQuantizer
    torch.manual_seed(0)
    vq = VectorQuantizer(32, 128, 0.25, vq_codebook_init_values=torch.randn(32, 128))
    vq.materialize_min_encodings = False
    return Shelgon("kvq-bert-tiny", vq, "kvq-bert-tiny", None, compute_dtype=torch.float32).cuda().eval()


def _data():
    g = torch.Generator().manual_seed(3)
    ids = torch.randint(1000, 2000, (8, 16), generator=g)
    lens = torch.randint(3, 17, (8,), generator=g)
    ids = ids * (torch.arange(16)[None] < lens[:, None])
    return ids.cuda(), (ids != 0).long().cuda()


def _same_on_all_ranks(t):
    import torch.distributed as dist
    raw = t.detach().contiguous().reshape(-1).view(torch.int32)
    hi, lo = raw.clone(), raw.clone()
    dist.all_reduce(hi, op=dist.ReduceOp.MAX)
    dist.all_reduce(lo, op=dist.ReduceOp.MIN)
    return bool(torch.equal(hi, lo))


def _worker(rank, world, port, out):
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), RANK=str(rank), WORLD_SIZE=str(world), LOCAL_RANK="0")
    os.environ.pop("KVQ_MAX_GRAD_NORM", None)
    sys.path.insert(0, os.path.join(ROOT, "kindergarten-vq-vae_amd"))
    import torch.distributed as dist
    from kvq import ddp
    from kvq.engine import TrainEngine
    torch.cuda.set_device(0)
    ddp.init_distributed("gloo")
    ids, mask = _data()
    half = slice(rank * 4, rank * 4 + 4)
    report = {}
    for tag, use_graph in (("eager", False), ("graph", True)):
        model = _build()
        ddp.broadcast_parameters(model)
        eng = TrainEngine(model, lr=1e-3, bucket_mib=0, max_grad_norm=0.25)       # bucket_mib=0: many chunks, a cut inside the buffer
        eng.use_graph = use_graph
        assert eng.world == 2 and eng._dp
        for step in range(1, STEPS + 1):
            res = eng.train_step(ids[half], mask[half])
            torch.cuda.synchronize()
            # the averaged gradient every rank holds after the step (clipping scales inside Adam, not in the buffer)
            want = sum((g.double() ** 2).sum().item() for g in eng.grads_by_parameter().values()) ** 0.5
            report[(tag, step)] = dict(norm=res["grad_norm"].item(), coef=res["grad_clip_coef"].item(), want=want,
                                       same_norm=_same_on_all_ranks(res["grad_norm"]), same_coef=_same_on_all_ranks(res["grad_clip_coef"]),
                                       same_master=_same_on_all_ranks(eng.flat.master), same_codebook=_same_on_all_ranks(eng.E.data),
                                       same_grad=_same_on_all_ranks(eng.flat.grad))
        report[tag + "_skipped"] = eng.skipped_steps
        if use_graph:
            assert len(eng._graphs) == 1
    if rank == 0:
        torch.save(report, out)
    dist.barrier()
    dist.destroy_process_group()


def _spawn_with_limit(fn, args, nprocs, limit_s):
    """mp.spawn whose workers are killed, and the test failed, when they are not done after limit_s seconds."""
    ctx = mp.spawn(fn, args=args, nprocs=nprocs, join=False)
    deadline = time.monotonic() + limit_s
    while not ctx.join(timeout=5.0):
        if time.monotonic() > deadline:
            for p in ctx.processes:
                if p.is_alive():
                    p.kill()
            pytest.fail(f"a data-parallel worker was not done after {limit_s} s")


def test_two_ranks_agree_on_the_norm_of_the_averaged_gradient(tmp_path):
    out = str(tmp_path / "dp_guard.pt")
    _spawn_with_limit(_worker, (2, _free_port(), out), 2, WORKER_LIMIT_S)
    rep = torch.load(out)
    for tag in ("eager", "graph"):
        assert rep[tag + "_skipped"] == 0
        for step in range(1, STEPS + 1):
            r = rep[(tag, step)]
            print(tag, step, r)
            bad = [k for k in ("same_norm", "same_coef", "same_master", "same_codebook", "same_grad") if not r[k]]
            assert not bad, f"{tag} step {step}: ranks differ in {bad}"
            assert abs(r["norm"] - r["want"]) <= 1e-6 * r["want"], (tag, step, r["norm"], r["want"])
            assert r["coef"] < 1.0                                        # clipping was active
