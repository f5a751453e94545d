"""Codebook revival over two data-parallel ranks (gloo, both on cuda:0), each training on its own half batch: usage is that of the
global batch (MAX all-reduce), a dead code's row comes from its owner rank alone (SUM all-reduce of one row and zeros), so codebook,
idle counters, moments and counter are bit-identical across the ranks, and every revived row is the restatement's pick from the
owner's donor source."""
import os
import socket
import sys
import time

import pytest
import torch
import torch.multiprocessing as mp

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
STEPS, T = 4, 2
K, H, B, S = 128, 128, 8, 8      # 2 x 32 tokens against 128 codes: at least 64 codes are dead from step T on
WORKER_LIMIT_S = 240          # per worker: two engines x four tiny steps + the process group (torch's import is most of it)


def _free_port():
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        return s.getsockname()[1]


def _build():
    sys.path.insert(0, os.path.join(ROOT, "kindergarten-vq-vae_amd"))
    from models.shelgon3.Shelgon import Shelgon
    from models.shelgon3.VectorQuantizer import VectorQuantizer
    torch.manual_seed(0)
    vq = VectorQuantizer(K, H, 0.25, vq_codebook_init_values=torch.randn(K, H), revive_after=T)
    vq.materialize_min_encodings = False
    return Shelgon("kvq-bert-tiny", vq, "kvq-bert-tiny", None, compute_dtype=torch.float32).cuda().eval()


def _data(step):
    g = torch.Generator().manual_seed(30 + step)
    ids = torch.randint(1000, 2000, (B, S), generator=g)
    lens = torch.randint(3, S + 1, (B,), generator=g)
    ids = ids * (torch.arange(S)[None] < lens[:, None])
    return ids.cuda(), (ids != 0).long().cuda()


def _same_on_all_ranks(t):
    import torch.distributed as dist
    raw = t.detach().contiguous().reshape(-1).view(torch.int32)
    hi, lo = raw.clone(), raw.clone()
    dist.all_reduce(hi, op=dist.ReduceOp.MAX)
    dist.all_reduce(lo, op=dist.ReduceOp.MIN)
    return bool(torch.equal(hi, lo))


def _gather(t):
    import torch.distributed as dist
    parts = [torch.empty_like(t) for _ in range(dist.get_world_size())]
    dist.all_gather(parts, t.contiguous())
    return parts


def _worker(rank, world, port, out):
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), RANK=str(rank), WORLD_SIZE=str(world), LOCAL_RANK="0")
    os.environ.pop("KVQ_VQ_REVIVE_AFTER", None)
    for p in (os.path.join(ROOT, "kindergarten-vq-vae_amd"), os.path.join(ROOT, "tests")):
        sys.path.insert(0, p)
    import numpy as np
    import torch.distributed as dist
    import _revive_ref as R
    from kvq import ddp
    from kvq.engine import TrainEngine
    torch.cuda.set_device(0)
    ddp.init_distributed("gloo")
    half = slice(rank * (B // 2), (rank + 1) * (B // 2))
    report = {}
    for tag, use_graph in (("eager", False), ("graph", True)):
        model = _build()
        ddp.broadcast_parameters(model)
        eng = TrainEngine(model, lr=1e-3)
        eng.use_graph = use_graph
        eng.revive_keep_donors = True
        assert eng.world == 2 and eng._dp and eng.revive_after == T
        idle = np.zeros((1, K), np.int32)
        total = 0
        for step in range(STEPS):
            ids, mask = _data(step)
            res = eng.train_step(ids[half], mask[half])
            torch.cuda.synchronize()
            a = eng.aux[0]
            same = {k: _same_on_all_ranks(t) for k, t in dict(E=eng.E.data, idle=eng.code_idle, m=a["m"], v=a["v"], counter=eng._rv_counter,
                                                              last=res["codes_revived"]).items()}
            # the restatement on the global batch: every rank's donor source and indices, gathered here
            donors = [d.float().cpu().numpy() for d in _gather(eng.revive_donors)]
            idx = torch.cat([i.reshape(-1) for i in _gather(res["indices"])]).cpu().numpy().reshape(1, -1)
            idle_sel, dead, rows, owner, _token = R.select(donors, R.usage_flags(idx, K), idle, T, eng._step_seed + step)
            idle = np.where(dead, 0, idle_sel).astype(np.int32)
            total += int(dead.sum())
            E = eng.E.detach().cpu().numpy().reshape(1, K, H)
            report[(tag, step)] = dict(same=same, last=int(res["codes_revived"].item()), want_last=int(dead.sum()),
                                       idle_ok=bool(np.array_equal(eng.code_idle.cpu().numpy(), idle)),
                                       rows_ok=bool(np.array_equal(R.bits(E[dead]), R.bits(rows[dead]))),
                                       owners=sorted(set(owner[dead].tolist())),
                                       moments_zero=not bool(a["m"].view(1, K, H)[torch.from_numpy(dead).cuda()].any()))
        report[tag + "_total"] = (eng.revived_codes, total)
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


def test_two_ranks_revive_the_same_codes_from_the_owners_rows(tmp_path):
    out = str(tmp_path / "dp_revive.pt")
    _spawn_with_limit(_worker, (2, _free_port(), out), 2, WORKER_LIMIT_S)
    rep = torch.load(out)
    for tag in ("eager", "graph"):
        got, want = rep[tag + "_total"]
        assert got == want > 0, (tag, got, want)
        owners = set()
        for step in range(STEPS):
            r = rep[(tag, step)]
            print(tag, step, r)
            bad = [k for k, ok in r["same"].items() if not ok]
            assert not bad, f"{tag} step {step}: ranks differ in {bad}"
            assert r["last"] == r["want_last"] and r["idle_ok"] and r["rows_ok"] and r["moments_zero"], (tag, step, r)
            owners.update(r["owners"])
        assert owners == {0, 1}, owners                              # both ranks donated rows
