"""TrainEngine -- the MI355X execution plan of one Shelgon / Bagon training step (models/shelgon3/Trainer.py:65-124).

The reference builds an autograd graph of ~2k ATen ops per step and lets torch.optim.Adam walk 400 parameter tensors.
This engine runs the same mathematics as an explicit forward / backward schedule over FLAT buffers:

  memory    every parameter of the model lives in one f32 master buffer (the nn.Parameters are re-pointed at views
            of it, so state_dict / checkpoints / the HF modules keep working), mirrored by one bf16 "shadow" buffer the
            GEMMs read, one bf16 gradient buffer the weight-gradient GEMMs write into directly, and f32 Adam moments.
            Q/K/V (and cross-attention K/V) weights are adjacent, so the fused [3H,H] projection is a plain view.
  forward   per block: one GEMM (+bias epilogue) -> one fused kernel (attention core | dropout+residual+LayerNorm | GELU)
  backward  hand-written mirror of forward; dropout masks are regenerated (Philox), never stored; bias gradients are
            column sums; weight gradients land in the flat gradient buffer with no accumulate/cast passes
  update    ONE Adam kernel over the flat buffers that also refreshes the bf16 shadow weights for the next step
  multi-GPU gradients are laid out in forward order, so backward finishes them from the end of the buffer towards
            the start: fixed-size tail chunks are all-reduced (RCCL, AVG, bf16) on a side stream while backward continues

GEMMs: every product of the bf16 step runs in libkvq.so -- csrc/kvq_gemm2.hip (LDS-DMA + MFMA; the tile is chosen by the cost
model kvq.nnops.pick_tile over (M, N, K), the persistent form by nnops.persistent_pays) or, for shapes that miss its divisibility /
alignment requirements, csrc/kvq_gemm_any.hip.  No vendor-library GEMM is reachable from a bf16 engine
(tests/test_engine_small_batches_gpu.py patches torch.mm / addmm / bmm / matmul to raise); the f32 engine, which exists as the
checker of the bf16 one, multiplies with torch (hipBLASLt, tuning/tunableop_gfx950.csv).
The calls outside the step -- attention maps, encode / decode, generation, beam search, reconstruction metrics -- are the mixin of
kvq/inference.py, which TrainEngine inherits.
Math restated from HuggingFace modeling_bert.py (see kvq/bert.py for the line map); tests/test_engine_gpu.py checks
losses and every parameter gradient against the autograd path (kvq.bert + torch autograd).
"""
from __future__ import annotations

import contextlib
import math
from typing import Dict, List, Tuple

import os

import torch
import torch.distributed as dist
import torch.nn.functional as F

from . import nnops
from ._ffi import FP8_E5M2, KvqError, check, io_dtype_of, lib, stream_ptr
from .functional import _workspace, check_revive_after, new_revive_counter, read_revive_counter, vq_revive_apply, vq_revive_select
from .inference import InferenceMixin, SamplingRefused, _round_up  # noqa: F401  (SamplingRefused: importable from here, as it was)

V_ALIGN = 64   # vocabulary rows of the LM head are padded so logits rows are 128-byte aligned

# model.__dict__["_kvq_engine"] = the engine that owns the model's flat buffers (Bagon / Shelgon.forward reuse it).  Model and
# engine reference each other, so the pair is collected together -- a registry keyed by the model would keep both alive
# (the engine holds the model strongly) together with ~4 GB of flat buffers at bert-base.
_QUANTIZERS = ("VectorQuantizer", "MultiVectorQuantizer", "GumbelQuantizer")


def engine_of(model, create=True):
    """The TrainEngine of `model` (its parameters live in that engine's flat buffers), created on first use."""
    eng = model.__dict__.get("_kvq_engine")
    if eng is not None and eng.flat.master.device != next(model.parameters()).device:
        eng = None                                         # the model was moved after the engine was built
    if eng is None and create:
        eng = TrainEngine(model)
    return eng


def fp8_span_table(offs, ns, n_total, span=2048):
    """span_segment of kvq_adam_step_dev_fp8 (include/kvq.h): for every `span`-element stretch of the flat parameter buffer the
    quantisation segment (offs[i], ns[i]) that covers ALL of it, -1 when no segment touches it, -2 when it holds a segment boundary
    (the kernel then walks the segment table for its 8 elements).  Segments must not overlap."""
    import numpy as np
    table = np.full((n_total + span - 1) // span, -1, dtype=np.int32)
    for si, (o, n) in enumerate(zip(offs, ns)):
        if n <= 0:
            continue
        k0, k1 = o // span, (o + n - 1) // span
        for k in range(k0, k1 + 1):
            lo, hi = span * k, min(span * k + span, n_total)
            whole = o <= lo and o + n >= hi
            table[k] = si if (whole and table[k] == -1) else -2
    return table


# ---- parameter groups and the learning-rate schedule: host side, plain Python / CPU tensors ---------------
# The BERT fine-tuning recipe as one line of a config: {"match": NO_DECAY, "weight_decay": 0.0} -- biases, LayerNorm gains and the
# LM-head bias take no weight decay.
NO_DECAY = ["*.b", "*.ln.w", "*.ln2.w", "head.bias"]
MAX_PARAM_GROUPS = 15          # beside group 0: kvq_adam_step_grouped holds 16 table entries


def resolve_param_groups(spec, names, default_wd):
    """spec: check_param_groups' list of {"match": [patterns], "lr_scale", "weight_decay" | None}; names: every parameter name of the
    engine, in its order.  Returns (table, group_of): table[j] = dict(group, match, lr_scale, weight_decay, names) with group 0 =
    what nothing matches (scale 1, default_wd), and group_of[name] = j.  First match wins (fnmatch, case-sensitive); a pattern that
    matches no name at all is refused by name -- a typo must not silently train under the defaults."""
    import fnmatch
    table = [dict(group=0, match=[], lr_scale=1.0, weight_decay=float(default_wd), names=[])]
    for j, g in enumerate(spec):
        for pat in g["match"]:
            if not any(fnmatch.fnmatchcase(n, pat) for n in names):
                raise KvqError(f"TrainEngine: param_groups[{j}]: the pattern {pat!r} matches no parameter name (param_names() lists them)")
        table.append(dict(group=j + 1, match=list(g["match"]), lr_scale=float(g["lr_scale"]),
                          weight_decay=float(default_wd if g["weight_decay"] is None else g["weight_decay"]), names=[]))
    group_of = {}
    for n in names:
        j = next((j + 1 for j, g in enumerate(spec) if any(fnmatch.fnmatchcase(n, pat) for pat in g["match"])), 0)
        group_of[n] = j
        table[j]["names"].append(n)
    return table, group_of


def param_group_blocks(layout, n_total, group_of):
    """block_group of kvq_adam_step_grouped as a CPU uint8 tensor of n_total / 16 entries.  layout: [(name, first element)] in buffer
    order, every first element and n_total a multiple of 16 (FlatParams); an entry owns the blocks up to the next entry's first one,
    its alignment padding included."""
    if n_total % 16 or any(o % 16 for _, o in layout):
        raise KvqError("param_group_blocks: entries must start at multiples of 16 elements")
    blocks = torch.zeros(n_total // 16, dtype=torch.uint8)
    ends = [o for _, o in layout[1:]] + [n_total]
    for (name, o), e in zip(layout, ends):
        if e < o:
            raise KvqError("param_group_blocks: the layout is not in buffer order")
        blocks[o // 16:e // 16] = group_of[name]
    return blocks


def range_group(blocks, a, b):
    """The group all blocks of the elements [a, b) share, or None when they hold more than one."""
    piece = blocks[a // 16:(b + 15) // 16]
    j = int(piece[0])
    return j if bool((piece == j).all()) else None


def lr_schedule_factor(t, warmup_steps, decay, total_steps, min_ratio):
    """warm * dec of kvq_step_state_advance_sched for the 1-based step t, as a Python float (the host mirror: TrainEngine._lr_now)."""
    W, r = int(warmup_steps), float(min_ratio)
    warm = t / W if W > 0 and t < W else 1.0
    if decay in (None, "none"):
        return warm
    x = min(max((t - W) / (int(total_steps) - W), 0.0), 1.0)
    return warm * (1.0 - (1.0 - r) * x if decay == "linear" else r + (1.0 - r) * 0.5 * (1.0 + math.cos(math.pi * x)))


class _EngineForward(torch.autograd.Function):
    """model.forward with autograd ON, on the engine's kernels: forward = TrainEngine.forward_backward(defer_backward=True),
    backward = TrainEngine.backward_from(d logits, d loss_vq).  The model's parameters are the function's inputs, so autograd
    accumulates into their .grad as for any other op.  (The ATen restatement kvq/bert.py stays the default when torch must
    differentiate: it is the independent checker of this schedule.  Opt in per model: model.autograd_backend = "engine".)"""

    @staticmethod
    def forward(ctx, eng, ids, mask, training, q_training, *params):
        out = eng.forward_backward(ids, mask, training=training, compute_grads=False, want_logits=True, quantizer_training=q_training,
                                   defer_backward=True)
        ctx.eng, ctx.resume, ctx.params = eng, out["_resume"], params
        logits = out["logits"]
        ctx.logits_shape = tuple(logits.shape)
        loss_vq = out["loss_vq_raw"] if out.get("loss_vq_raw") is not None else torch.zeros((), device=logits.device)
        perp = out["perplexity"] if out.get("perplexity") is not None else torch.zeros((), device=logits.device)
        idx = out["indices"] if out.get("indices") is not None else torch.zeros(0, dtype=torch.int64, device=logits.device)
        loss_vq, perp = loss_vq.clone(), perp.clone()          # (views of one two-element result buffer otherwise)
        ctx.mark_non_differentiable(perp, idx)
        return logits, loss_vq, perp, idx

    @staticmethod
    def backward(ctx, g_logits, g_loss_vq, _g_perp, _g_idx):
        eng = ctx.eng
        if g_logits is None:                                   # a loss of the quantiser term alone
            g_logits = torch.zeros(ctx.logits_shape, device=eng.dev, dtype=eng.dtype)
        eng.backward_from(ctx.resume, g_logits.to(eng.dtype), g_loss_vq)
        by_p = eng.grads_by_parameter()
        return (None, None, None, None, None) + tuple(by_p.get(p) if p.requires_grad else None for p in ctx.params)


def engine_autograd_forward(model, ids, mask, q_training=None):
    """(logits [B, S, V], loss_vq (unweighted), perplexity, indices) of `model` with an autograd edge to every parameter."""
    eng = engine_of(model)
    eng.refresh_if_params_changed()
    params = tuple(p for p in model.parameters())
    return _EngineForward.apply(eng, ids, mask, model.training, q_training, *params)


_TUNING_LOADED = False


def _load_gemm_tuning():
    """hipBLASLt/rocBLAS solution choices for this step's GEMM shapes, tuned once on an MI355X with PyTorch's TunableOp
    and shipped in tuning/ (a lookup table of library solution ids; no tuning happens at run time).  Shapes not in the
    table use the library's default heuristic."""
    global _TUNING_LOADED
    if _TUNING_LOADED:
        return
    _TUNING_LOADED = True
    import os
    path = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tuning", "tunableop_gfx950.csv")
    if os.environ.get("KVQ_GEMM_TUNING", "1") == "0" or not os.path.exists(path):
        return
    try:
        import torch.cuda.tunable as tn
        tn.enable(True)
        tn.tuning_enable(os.environ.get("KVQ_GEMM_TUNING") == "tune")
        if os.environ.get("KVQ_GEMM_TUNING") == "tune":
            tn.set_filename(os.environ.get("KVQ_GEMM_TUNING_OUT", "gpurun_out/tunableop_new.csv"), False)
            tn.set_max_tuning_duration(int(os.environ.get("KVQ_GEMM_TUNING_MS", 15)))
            if os.environ.get("KVQ_GEMM_TUNING_ITERS"):
                tn.set_max_tuning_iterations(int(os.environ["KVQ_GEMM_TUNING_ITERS"]))
        else:
            tn.read_file(path)
            if hasattr(tn, "write_file_on_exit"):
                tn.write_file_on_exit(False)
    except Exception as e:   # tuning tables are an optimisation only
        print(f"[kvq] GEMM tuning table not loaded: {e}")


class FlatParams:
    """Flat master / shadow / gradient / moment buffers over a list of (name, parameter, padded_numel)."""

    def __init__(self, entries: List[Tuple[str, torch.nn.Parameter, int]], device, compute_dtype, amsgrad: bool):
        self.compute_dtype = compute_dtype
        self.seg: Dict[str, Tuple[int, int, torch.Size]] = {}
        self.trainable: Dict[str, bool] = {}
        off = 0
        for name, p, padded in entries:
            self.seg[name] = (off, p.numel(), p.shape)
            self.trainable[name] = p.requires_grad
            off += _round_up(padded, 16)       # 16 elements: an fp8 mirror of a segment stays 16-byte aligned
        self.n = _round_up(off, 16)
        self.master = torch.zeros(self.n, dtype=torch.float32, device=device)
        for name, p, _ in entries:
            o, n, shape = self.seg[name]
            self.master[o:o + n].copy_(p.data.reshape(-1))
            p.data = self.master[o:o + n].view(shape)          # the module's parameter IS the master copy now
        if compute_dtype == torch.float32:
            self.shadow = self.master
        else:
            self.shadow = self.master.to(compute_dtype)
        # gradient and Adam-moment buffers on first use: an engine that only ever serves Bagon / Shelgon.forward (no autograd,
        # engine_of(model)) never touches them -- 2.5 of the 4.5 GB of flat buffers at bert-base.  The first training steps run
        # eagerly, so the allocation never falls inside a hipGraph capture.
        self._device, self._amsgrad = device, amsgrad
        self._grad = self._m = self._v = self._vmax = self._acc = self._ema = None
        # contiguous trainable ranges (Adam is launched once per range; one range in `full` mode)
        self.ranges: List[Tuple[int, int]] = []
        for name, p, padded in entries:
            if not p.requires_grad:
                continue
            o = self.seg[name][0]
            e = o + _round_up(padded, 16)
            if self.ranges and self.ranges[-1][1] == o:
                self.ranges[-1] = (self.ranges[-1][0], e)
            else:
                self.ranges.append((o, e))

        # the trainable PARAMETER elements as contiguous pieces: the ranges without the alignment padding behind an entry and the
        # padded rows of the vocabulary table (what a global gradient norm runs over; every piece starts at a multiple of 16)
        self.pieces: List[Tuple[int, int]] = []
        for name, p, padded in entries:
            if not p.requires_grad or p.numel() == 0:
                continue
            o, n, _ = self.seg[name]
            if self.pieces and self.pieces[-1][1] == o:
                self.pieces[-1] = (self.pieces[-1][0], o + n)
            else:
                self.pieces.append((o, o + n))

    def _lazy(self, attr, dtype):
        t = getattr(self, attr)
        if t is None:
            t = torch.zeros(self.n, dtype=dtype, device=self._device)
            setattr(self, attr, t)
        return t

    @property
    def grad(self):
        return self._lazy("_grad", self.compute_dtype)

    @property
    def m(self):
        return self._lazy("_m", torch.float32)

    @property
    def v(self):
        return self._lazy("_v", torch.float32)

    @property
    def vmax(self):
        return self._lazy("_vmax", torch.float32) if self._amsgrad else None

    @property
    def acc(self):
        """f32 sum / mean of the micro-batch gradients (TrainEngine(grad_accum > 1) only: nothing else touches it)."""
        return self._lazy("_acc", torch.float32)

    @property
    def ema(self):
        """f32 moving average of the master buffer over the trainable ranges (TrainEngine(weight_ema=...) only: nothing else touches
        it; a frozen element is never written and never read)."""
        return self._lazy("_ema", torch.float32)

    def optimizer_state_allocated(self) -> bool:
        return self._grad is not None or self._m is not None or self._v is not None

    def w(self, name, rows=None):
        o, n, shape = self.seg[name]
        if rows is not None:                                       # padded 2-D view [rows, shape[1]]
            return self.shadow[o:o + rows * shape[1]].view(rows, shape[1])
        return self.shadow[o:o + n].view(shape)

    def g(self, name, rows=None):
        o, n, shape = self.seg[name]
        if rows is not None:
            return self.grad[o:o + rows * shape[-1]].view(rows, shape[-1]) if len(shape) > 1 else self.grad[o:o + rows]
        return self.grad[o:o + n].view(shape)

    def w32(self, name):
        o, n, shape = self.seg[name]
        return self.master[o:o + n].view(shape)

    def fused(self, names, buf):
        """View spanning adjacent segments (e.g. q,k,v weights) as one [sum rows, cols] matrix / [sum] vector."""
        o0, _, shape0 = self.seg[names[0]]
        total = 0
        for nm in names:
            o, n, _ = self.seg[nm]
            assert o == o0 + total, f"segments {names} are not adjacent"
            total += n
        flat = buf[o0:o0 + total]
        return flat.view(-1, shape0[1]) if len(shape0) == 2 else flat

    def refresh_shadow(self):
        if self.shadow is not self.master:
            self.shadow.copy_(self.master)


class _StepGraphs:
    """One training step of a fixed batch shape as a chain of hipGraphs with eager launches in between.

    The step is captured once; wherever the engine has something that must stay an ordinary launch it calls interlude(fn):
    the running capture ends, fn is kept (and run once), the next capture begins in the same memory pool.  Interludes are
      * the quantiser forward (kvq_vq_forward: the kernel bench.py times with HIP events on every launch), and
      * on multi-GPU runs every gradient all-reduce (RCCL, issued on the side stream while the next graph runs) and the
        final wait for them before the Adam graph.
    Replay = graph, interlude, graph, ...: ~3 host launches per step on one GPU instead of ~800.  Nothing inside the graphs
    depends on host values that change between steps: see the device step state in include/kvq.h."""

    def __init__(self, eng, ids, mask, dec=None, final=True):
        self.eng = eng
        dev = eng.dev
        self.final = final      # grad_accum > 1: False = a micro chain (forward, backward, accumulate, advance), True = the same plus the optimiser
        # static input buffers the captured kernels read: ids | mask | ids sorted (stable, pads under -1) | their order
        # [| the decoder's own ids | mask | sorted | order | the loss target -- a Bagon step, models/bagon/Trainer.py:65-130]
        self.pack = eng.pack_batch(ids, mask, *(dec or ())).reshape(-1)
        N, H = ids.numel(), eng.H
        self.ids, self.mask, srt, perm, self.dec = eng.unpack_batch(self.pack, ids.shape, dec[0].shape if dec else None)
        self.sorted = (srt, perm)
        self.z_q = torch.empty((N, H), dtype=eng.dtype, device=dev)
        self.idx = torch.empty(N * max(eng.G, 1), dtype=torch.int64, device=dev)
        # loss, accuracy | quantiser loss, perplexity | counted tokens (loss_ignore_pad; 0 otherwise): one clone per step
        self.scal = torch.zeros(5, dtype=torch.float32, device=dev)
        self.vq_out = self.scal[2:4]
        # keep_graph: the captured hipGraph_t stays readable behind the executable one (node_census; a few hundred nodes)
        self.graphs, self.inter = [torch.cuda.CUDAGraph(keep_graph=True)], []
        side = torch.cuda.Stream(device=dev)
        # no garbage collection while a capture is open (what torch.cuda.graph does as well): a collected cycle may own HIP
        # objects -- an older engine's kept hipGraphs -- whose destruction is not permitted while this thread captures
        import gc
        gc_was_on = gc.isenabled()
        step0 = eng._step_host
        try:
            gc.collect()
            gc.disable()
            torch.cuda.synchronize(dev)
            side.wait_stream(torch.cuda.current_stream(dev))
            with torch.cuda.stream(side):
                eng._cap = self
                ok = False
                try:
                    # thread-local capture mode: the process group's helper threads (gloo copies, the RCCL watchdog's event
                    # queries) keep issuing HIP calls on their own streams while this thread captures
                    self.graphs[0].capture_begin(capture_error_mode="thread_local")
                    eng._prepared = dict(enc=self.sorted, dec=self.dec[2:4] if self.dec else None)
                    dkw = dict(dec_ids=self.dec[0], dec_mask=self.dec[1], target_ids=self.dec[4]) if self.dec else {}
                    self.out = eng.forward_backward(self.ids, self.mask, training=eng.model.training, compute_grads=True, **dkw)
                    self.fp8_bwd = (eng.fp8_bwd_launches, list(eng.fp8_bwd_sites))      # what THIS chain holds: restored by every replay
                    eng._finish_step(final)
                    self.graphs[-1].capture_end()
                    if eng._guard is not None and final:      # grad_norm / grad_clip_coef: views of the guard state, run() hands out copies
                        self.out.update(eng._guard_out)
                    if eng.revive_after is not None and final:
                        self.out["codes_revived"] = eng._rv_counter[0]
                    if eng.weight_ema is not None and final:
                        self.out["weight_ema_decay"] = eng._wema_out
                    if eng.lr_schedule is not None and final:      # the rate of the step just applied, a view of the step state
                        self.out["lr"] = eng._lr_out
                    ok = True
                finally:
                    eng._cap = None
                    eng._prepared = None
                    eng._step_host = step0      # capturing ran no captured kernel: the device step state did not move either
                                                # (nor the accumulation state: its host mirror is train_step's alone)
                    if not ok:                  # close the capture that was open when the error struck
                        try:
                            self.graphs[-1].capture_end()
                        except Exception:
                            pass
        finally:
            if gc_was_on:
                gc.enable()
        torch.cuda.current_stream(dev).wait_stream(side)
        torch.cuda.synchronize(dev)

    def interlude(self, fn):
        """Called by the engine in the middle of the captured step: fn stays an eager launch between two graphs."""
        self.graphs[-1].capture_end()
        fn()
        self.inter.append(fn)
        g = torch.cuda.CUDAGraph(keep_graph=True)
        g.capture_begin(pool=self.graphs[0].pool(), capture_error_mode="thread_local")
        self.graphs.append(g)

    def node_census(self):
        """Per captured graph of the chain: {kind: nodes} (kvq_graph_census).  A step graph must consist of kernel nodes (and the
        empty / event nodes of a stream fork) only: a memset or memcpy node is a launch of another kind whose order against the
        neighbouring kernel nodes this stack did not keep (profiles/r04_fp8.md) -- tests/test_graph_nodes_gpu.py."""
        import ctypes
        kinds = ("kernel", "memset", "memcpy", "empty", "event", "other")
        out = []
        for g in self.graphs:
            counts = (ctypes.c_int64 * len(kinds))()
            check(lib().kvq_graph_census(g.raw_cuda_graph(), counts), "kvq_graph_census")
            out.append(dict(zip(kinds, (int(c) for c in counts))))
        return out

    def run(self, ids, mask, prep, dec=None):
        """prep: TrainEngine._normalise_prepared()'s dict (pack = the whole batch as one tensor, or the sorted ids of either side)."""
        self.eng.fp8_bwd_launches, self.eng.fp8_bwd_sites = self.fp8_bwd[0], list(self.fp8_bwd[1])
        if prep["pack"] is not None:
            self.pack.copy_(prep["pack"])           # a batch packed where it was built (TrainEngine.pack_batch): one copy
        else:                                       # otherwise the sort happens here -- outside the graphs, but in the step
            self.ids.copy_(ids)
            self.mask.copy_(mask)
            srt, perm = prep["enc"] if prep["enc"] is not None else self.eng.prepare_batch(ids)
            self.sorted[0].copy_(srt)
            self.sorted[1].copy_(perm)
            if self.dec:
                d_ids, d_mask, tgt = dec
                self.dec[0].copy_(d_ids)
                self.dec[1].copy_(d_mask)
                srt, perm = prep["dec"] if prep["dec"] is not None else self.eng.prepare_batch(d_ids)
                self.dec[2].copy_(srt)
                self.dec[3].copy_(perm)
                self.dec[4].copy_(d_ids if tgt is None else tgt)
        for i, g in enumerate(self.graphs):
            g.replay()
            if i < len(self.inter):
                self.inter[i]()
        self.eng._step_host += int(self.final)
        # the graph's buffers are overwritten by the next step: hand out copies (the four scalars as views of ONE copy)
        sc = self.scal.clone()
        res = {}
        for k, v in self.out.items():
            if v is None:
                res[k] = None
            elif v.untyped_storage().data_ptr() == self.scal.untyped_storage().data_ptr():
                res[k] = sc[v.storage_offset()]
            else:
                res[k] = v.clone()
        return res


class TrainEngine(InferenceMixin):
    def __init__(self, model, lr=1e-4, betas=(0.9, 0.999), eps=1e-8, weight_decay=0.0, amsgrad=False,
                 milestones=None, gamma=0.1, loss_recon_scale=1.0, loss_vq_scale=1.0, seed=1234,
                 bucket_mib=64, process_group=None, fp8_forward=None, fp8_backward=None, max_grad_norm=None, grad_accum=None,
                 weight_ema=None, loss_ignore_pad=None, param_groups=None, decoupled_weight_decay=None, lr_warmup_steps=None,
                 lr_decay=None, lr_total_steps=None, lr_min_ratio=None):
        self.model = model
        # options, off by default: parameter groups, AdamW's decoupled decay, warm-up / decay of the rate
        self._pg_spec = self.check_param_groups(param_groups, env=True)
        self.decoupled_wd = self.check_decoupled_weight_decay(decoupled_weight_decay, env=True)
        self.lr_schedule = self.check_lr_schedule(self.check_lr_warmup_steps(lr_warmup_steps, env=True),
                                                  self.check_lr_decay(lr_decay, env=True),
                                                  self.check_lr_total_steps(lr_total_steps, env=True),
                                                  self.check_lr_min_ratio(lr_min_ratio, env=True))
        if (self._pg_spec is not None or self.decoupled_wd) and (isinstance(weight_decay, bool) or not isinstance(weight_decay, (int, float))
                                                                 or not 0 <= weight_decay < math.inf):      # (it fills the group table)
            raise KvqError(f"TrainEngine: param_groups / decoupled_weight_decay need a finite weight_decay >= 0, got {weight_decay!r}")
        self.loss_ignore_pad = self.check_loss_ignore_pad(loss_ignore_pad, env=True)
        self.grad_accum = self.check_grad_accum(grad_accum, env=True)
        self.max_grad_norm = self.check_max_grad_norm(max_grad_norm, env=True)     # (before anything is laid out: a bad value changes nothing)
        self.weight_ema = self.check_weight_ema(weight_ema, env=True)
        # option, off by default: codebook revival.  The quantiser's revive_after; None there: KVQ_VQ_REVIVE_AFTER
        # from the environment, as max_grad_norm reads KVQ_MAX_GRAD_NORM (unset / empty: off).  A model without a quantiser ignores it.
        self.revive_after = None
        if hasattr(model, "vector_quantizer"):
            self.revive_after = check_revive_after(getattr(model.vector_quantizer, "revive_after", None), env=True)
        if self.grad_accum > 1:           # refused before anything is laid out; each combination is a piece of work of its own
            if process_group is not None or os.environ.get("KVQ_DP_SINGLE_RANK", "0") == "1" \
                    or (dist.is_initialized() and dist.get_world_size(process_group) > 1):
                raise KvqError("TrainEngine: grad_accum > 1 with data parallelism (a process group / KVQ_DP_SINGLE_RANK): the gradient "
                               "exchange would have to move to the accumulator and run on the last micro-step only")
            if self.revive_after is not None:
                raise KvqError("TrainEngine: grad_accum > 1 with codebook revival (revive_after / KVQ_VQ_REVIVE_AFTER): the usage "
                               "flags would have to be OR-ed over the micro-steps of a cycle")
            if getattr(getattr(model, "vector_quantizer", None), "ema_decay", None) is not None:
                raise KvqError("TrainEngine: grad_accum > 1 with an EMA codebook (ema_decay): its statistics would have to be summed "
                               "over the micro-steps of a cycle")
        dev = next(model.parameters()).device
        if dev.type != "cuda":
            raise KvqError("TrainEngine needs the model on an MI355X (there is no CPU path)")
        lib()
        self.dev = dev
        self.dtype = model.compute_dtype
        self.io = 1 if self.dtype == torch.bfloat16 else 0
        self.has_vq = hasattr(model, "vector_quantizer")
        self.sentence_acc = not self.has_vq       # the plain Bagon step reports the accuracy of every sentence as well
        self.vq_kind = type(model.vector_quantizer).__name__ if self.has_vq else None
        if self.has_vq and self.vq_kind not in _QUANTIZERS:
            raise KvqError(f"TrainEngine schedules {', '.join(_QUANTIZERS)}; got {self.vq_kind}")
        self.G = 1
        enc, dec = model.encoder, model.decoder
        self.ecfg, self.dcfg = enc.config, dec.config
        if self.ecfg.hidden_size // self.ecfg.num_attention_heads != 64:
            raise KvqError("TrainEngine: attention kernels are written for head dim 64")
        self.H = self.ecfg.hidden_size
        self.V = self.dcfg.vocab_size
        self.Vp = _round_up(self.V, V_ALIGN)
        self.lr, self.betas, self.eps, self.wd = lr, betas, eps, weight_decay
        self.milestones, self.gamma = sorted(milestones or []), gamma
        self.w_recon, self.w_vq = float(loss_recon_scale), float(loss_vq_scale)
        self.seed = int(seed)
        if len(self.milestones) > 8:
            raise KvqError("TrainEngine: at most 8 LR milestones (kvq_step_state_advance)")
        # what changes from step to step lives on the device (include/kvq.h "step state"): dropout kernels add the step count
        # to their seed, Adam reads lr and the bias corrections -- so a captured hipGraph of the whole step can be replayed
        self._state = nnops.new_step_state(dev)
        self._step_host = 0
        self._step_seed = (self.seed * 1000003) & 0x7FFFFFFFFFFFFFF      # + step count on the device
        self._graphs, self._eager_seen, self._cap, self._prepared = {}, {}, None, None
        self._maps = None                  # attention_maps() only: where _attn_block_fwd leaves the probabilities
        self._own_fwd = os.environ.get("KVQ_OWN_GEMM", "1") != "0"
        self._gumbel_own = 0                  # products of the Gumbel mode that ran on the own GEMM (tests read it)
        if os.environ.get("KVQ_GEMM_TILE"):       # "NxK:tile;NxK:tile" (A/B runs on the GPU box)
            self._TILE_OVERRIDE = {tuple(int(v) for v in e.split(":")[0].split("x")): e.split(":")[1]
                                   for e in os.environ["KVQ_GEMM_TILE"].split(";") if e}
        # round 5: dropout + residual of a BertSelfOutput / BertOutput block in the dense layer's epilogue, LayerNorm alone behind it
        # (8.2 us instead of 11.9: one tensor read, one written).  Bit-identical -- and only worth it WITHOUT dropout: the Philox
        # rounds of 6 M elements are ~5 us of vector-ALU time per SIMD, which the LayerNorm kernel hides behind its loads and a
        # GEMM epilogue does not (same-box traces, profiles/r05_gemm_ceiling.md: +7 us per GEMM against -3.7 us per LayerNorm).
        # "eval" (default): steps without dropout (validation / test stages, model.forward); "1": always (tests); "0": never.
        self._fuse_dropres = os.environ.get("KVQ_FUSE_DROPRES", "eval")
        # weight gradients as grouped launches of csrc/kvq_gemm2.hip, two layers per launch where they fit one round of the CUs
        # (_flush_wgrads)
        self._own_wgrad = self._own_fwd and self.dtype == torch.bfloat16
        self._wg_pack = False                 # the packed schedule (one process only): set below, once _dp is known
        self._n_cu = nnops.cu_count(dev)
        self._wg_reset()
        # LM head + the loss' forward statistics in one kernel (see _forward_backward): built and parity-tested in round 2, and
        # 0.08 ms/step SLOWER than library GEMM + kvq_ce_forward (18.55 against 18.47 ms, gpurun_out/ab16.log): opt-in
        self._own_lmce = os.environ.get("KVQ_OWN_LMCE", "0") == "1"
        self.use_graph = os.environ.get("KVQ_GRAPH", "1") != "0"
        self.group = process_group
        self.world = dist.get_world_size(process_group) if dist.is_initialized() else 1
        # the gradient exchange runs when there is more than one rank -- or, for a rehearsal of the RCCL branch on a one-GPU box,
        # with a ONE-rank process group and KVQ_DP_SINGLE_RANK=1 (every all-reduce, stream hand-over and graph interlude executes;
        # the averages are over one rank)
        self._dp = self.world > 1 or (dist.is_initialized() and os.environ.get("KVQ_DP_SINGLE_RANK", "0") == "1")
        # KVQ_WG_PACK=0: the unpacked weight-gradient schedule (A/B switch); with a process group always -- _wg_done_lo is one
        # watermark that takes gradients to become final in buffer order, which the packed schedule's late cross-K/V slices are not
        self._wg_pack = self._own_wgrad and not self._dp and os.environ.get("KVQ_WG_PACK", "1") != "0"

        # ---- flat parameter layout, in FORWARD order (gradients then complete from the tail backwards)
        entries, seen = [], set()
        self.param_of: Dict[str, torch.nn.Parameter] = {}

        def add(name, p, padded=None):
            if id(p) in seen:
                return
            seen.add(id(p))
            self.param_of[name] = p
            entries.append((name, p, padded if padded is not None else p.numel()))

        def add_emb(prefix, emb, pad_word_rows=None):
            w = emb.word_embeddings.weight
            add(prefix + "word", w, (pad_word_rows or w.shape[0]) * w.shape[1])
            add(prefix + "pos", emb.position_embeddings.weight)
            add(prefix + "type", emb.token_type_embeddings.weight)
            add(prefix + "ln.w", emb.LayerNorm.weight); add(prefix + "ln.b", emb.LayerNorm.bias)

        def add_attn(prefix, att, cross):
            s = att.self
            if cross:
                add(prefix + "q.w", s.query.weight)
                add(prefix + "k.w", s.key.weight); add(prefix + "v.w", s.value.weight)
                add(prefix + "q.b", s.query.bias)
                add(prefix + "k.b", s.key.bias); add(prefix + "v.b", s.value.bias)
            else:
                add(prefix + "q.w", s.query.weight); add(prefix + "k.w", s.key.weight); add(prefix + "v.w", s.value.weight)
                add(prefix + "q.b", s.query.bias); add(prefix + "k.b", s.key.bias); add(prefix + "v.b", s.value.bias)
            add(prefix + "o.w", att.output.dense.weight); add(prefix + "o.b", att.output.dense.bias)
            add(prefix + "ln.w", att.output.LayerNorm.weight); add(prefix + "ln.b", att.output.LayerNorm.bias)

        def add_layer(prefix, layer, cross):
            add_attn(prefix + "sa.", layer.attention, False)
            if cross:
                add_attn(prefix + "ca.", layer.crossattention, True)
            add(prefix + "f1.w", layer.intermediate.dense.weight); add(prefix + "f1.b", layer.intermediate.dense.bias)
            add(prefix + "f2.w", layer.output.dense.weight); add(prefix + "f2.b", layer.output.dense.bias)
            add(prefix + "ln2.w", layer.output.LayerNorm.weight); add(prefix + "ln2.b", layer.output.LayerNorm.bias)

        add_emb("enc.emb.", enc.embeddings)
        for i, layer in enumerate(enc.encoder.layer):
            add_layer(f"enc.{i}.", layer, False)
        add_emb("dec.emb.", dec.bert.embeddings, pad_word_rows=self.Vp)     # tied to the LM head: padded to Vp rows
        # Every decoder layer projects the SAME encoder output (the quantised z_q) to its cross-attention keys / values
        # (modeling_bert.py:83-85 with encoder_hidden_states): their weights sit side by side so that the 12 projections, their
        # input gradients and their weight gradients each run as ONE GEMM over [L*2H, H] instead of 12 narrow ones.
        dlayers = list(dec.bert.encoder.layer)
        self._cakv_w = [n for i in range(len(dlayers)) for n in (f"dec.{i}.ca.k.w", f"dec.{i}.ca.v.w")]
        self._cakv_b = [n for i in range(len(dlayers)) for n in (f"dec.{i}.ca.k.b", f"dec.{i}.ca.v.b")]
        for i, layer in enumerate(dlayers):
            sx = layer.crossattention.self
            add(f"dec.{i}.ca.k.w", sx.key.weight); add(f"dec.{i}.ca.v.w", sx.value.weight)
        for i, layer in enumerate(dlayers):
            sx = layer.crossattention.self
            add(f"dec.{i}.ca.k.b", sx.key.bias); add(f"dec.{i}.ca.v.b", sx.value.bias)
        for i, layer in enumerate(dlayers):
            add_layer(f"dec.{i}.", layer, True)
        head = dec.cls.predictions
        add("head.t.w", head.transform.dense.weight); add("head.t.b", head.transform.dense.bias)
        add("head.ln.w", head.transform.LayerNorm.weight); add("head.ln.b", head.transform.LayerNorm.bias)
        add("head.bias", head.decoder.bias, self.Vp)
        if head.decoder.weight is not dec.bert.embeddings.word_embeddings.weight:
            raise KvqError("TrainEngine expects the LM head tied to the decoder word embeddings (HF default)")
        # names of the parameters outside the flat buffers (codebook, Gumbel projection / embedding), then the parameter groups: resolved
        # BEFORE anything is laid out -- an unknown pattern changes nothing
        self._aux_names = {"VectorQuantizer": ["vq.codebook"], "MultiVectorQuantizer": ["vq.codebook"],
                           "GumbelQuantizer": ["vq.proj.weight", "vq.proj.bias", "vq.embed.weight"]}.get(self.vq_kind, [])
        self._pg = None
        if self._pg_spec is not None or self.decoupled_wd:
            table, group_of = resolve_param_groups(self._pg_spec or [], [e[0] for e in entries] + self._aux_names, weight_decay)
            self._pg = dict(table=table, group_of=group_of)
        # parameters the step never touches (pooler) stay outside the flat buffers and receive no gradient
        self.flat = FlatParams(entries, dev, self.dtype, amsgrad)
        pads = {enc.embeddings.word_embeddings.padding_idx, dec.bert.embeddings.word_embeddings.padding_idx}
        if len(pads) != 1:
            raise KvqError("TrainEngine expects the same padding_idx in the encoder and decoder word embeddings")
        self._pad_idx = pads.pop()
        # option, off by default: reconstruction loss, accuracy and per-sentence accuracy over the tokens whose
        # target is not the pad id (F.cross_entropy's ignore_index) -- the kvq_*_ignore entry points of the loss kernels
        if self.loss_ignore_pad and self._pad_idx is None:
            raise KvqError("TrainEngine: loss_ignore_pad (KVQ_LOSS_IGNORE_PAD) needs word embeddings with a padding_idx: there is no "
                           "pad id to leave out of the loss")
        self.n_enc_layers = len(enc.encoder.layer)
        self.n_dec_layers = len(dec.bert.encoder.layer)
        self.nh = self.ecfg.num_attention_heads
        flags = {self.flat.trainable[n] for n in self._cakv_w + self._cakv_b}
        self._cakv_batched = len(flags) == 1 and self.n_dec_layers > 0       # mixed frozen / trained layers: per-layer GEMMs
        # small f32 parameters outside the flat buffers (codebook, Gumbel projection / embedding): own gradient + Adam state
        self.aux = []
        self._bufs = {}
        self._gen_cache = {}              # generate(): buffers and captured step per (B, Se, max_length, want_logits)
        self._beam_cache = {}             # beam_search(): the same per (B, Se, max_length, num_beams, want_trace)

        def add_aux(p, name):
            a = dict(name=name, p=p, g=torch.zeros_like(p.data), m=torch.zeros_like(p.data), v=torch.zeros_like(p.data),
                     vmax=torch.zeros_like(p.data) if amsgrad else None)
            self.aux.append(a)
            return a["g"]

        self.vq_ema = False
        if self.vq_kind in ("VectorQuantizer", "MultiVectorQuantizer"):
            vq = model.vector_quantizer
            self.G = int(getattr(vq, "n_factors", 1))         # codebooks = slices of the encoder output, one grouped launch
            self.K, self.Dg = int(vq.n_e), int(getattr(vq, "d_factor", self.H))       # (padded) slice width
            self.E = vq.embedding.weight                      # f32 [G*K, H/G]
            if self.E.shape != (self.G * self.K, self.Dg):
                raise KvqError(f"TrainEngine: codebook {tuple(self.E.shape)} does not match {self.G} x {self.K} x {self.Dg}")
            self.beta_vq = float(vq.beta)
            self.vq_ema = getattr(vq, "ema_decay", None) is not None     # extension: EMA codebook update instead of the gradient
            self.gE = add_aux(self.E, "vq.codebook") if self.E.requires_grad else torch.zeros_like(self.E.data)
            # the codebook in MFMA-fragment order (kvq_vq_pack_codebook): rebuilt after every codebook update -- Adam at the end
            # of the step, the EMA step, or a write from outside (noticed through the tensor version) -- not per forward call
            self._epack = torch.empty(lib().kvq_vq_packed_bytes(self.K, self.Dg, self.G), dtype=torch.uint8, device=dev) \
                if self.Dg % 32 == 0 else None
            self._E_version = None
        elif self.vq_kind == "GumbelQuantizer":
            if self.revive_after is not None:
                raise KvqError("TrainEngine: codebook revival (revive_after / KVQ_VQ_REVIVE_AFTER) is defined for the arg-min "
                               "quantisers, not for GumbelQuantizer")
            gq = model.vector_quantizer
            if gq.n_embed > 1024:
                raise KvqError("TrainEngine: the Gumbel row kernel holds at most 1024 codes")
            self.g_pw, self.g_pb, self.g_emb = (add_aux(gq.proj.weight, "vq.proj.weight"), add_aux(gq.proj.bias, "vq.proj.bias"),
                                                add_aux(gq.embed.weight, "vq.embed.weight"))
        # extension (BASELINE.json configs[4], default off): forward GEMMs on the fp8 matrix cores; per-tensor scales -- weights from
        # the tensor itself after every update, activations delayed by one training step (kvq_fp8_quantize_delayed).
        # True / KVQ_FP8=1: the products where fp8 + the activation's quantisation pass beat the own bf16 kernel -- outputs at least
        # _FP8_MIN_ROWS wide: the LM head and the all-layer cross-K/V projection (tools/gemm2_probe_fp8_own.py, profiles/r04_fp8.md:
        # 292 against 350 us and 184 against 217; every per-layer GEMM LOSES 4 - 8 us to its quantisation pass).
        # "all" / KVQ_FP8=all: every forward GEMM (rounds 2 - 3; kept for the numerics tests and as the A/B arm).
        # "fused" / KVQ_FP8=fused (round 5): every forward GEMM of the layers, each reading an fp8 copy of its input that the kernel
        # PRODUCING that input wrote beside the bf16 one (LayerNorm forward, attention forward, the GELU epilogue of the fp8
        # BertIntermediate GEMM: kvq_*_fp8) -- the 120 quantisation passes of "all" are gone; what still takes a pass is the input
        # of a layer-0 QKV projection (embedding kernel) and of the cross-K/V projection (quantiser output).
        # Since round 5 this is what fp8_forward=True / KVQ_FP8=1 means (same box, nine codebooks, profiles/r05_fp8.md: 16.96 ms against
        # 17.05 for "wide" and 17.14 for bf16); "wide" = rounds 4's two GEMMs, "all" = every GEMM behind a quantisation pass (A/B arm).
        if fp8_forward is None:
            fp8_forward = {"0": False, "1": True, "all": "all", "fused": "fused", "wide": "wide"}.get(os.environ.get("KVQ_FP8", "0"), False)
        if fp8_forward is True:
            fp8_forward = "fused"
        if fp8_forward not in (False, "fused", "wide", "all"):
            raise KvqError(f"TrainEngine: fp8_forward must be False, True / \"fused\", \"wide\" or \"all\", got {fp8_forward!r}")
        self.fp8 = bool(fp8_forward)
        if self.fp8 and self.weight_ema is not None:
            raise KvqError("TrainEngine: weight_ema with fp8 forward GEMMs (fp8_forward / KVQ_FP8): evaluation under the average swaps "
                           "the weights, and their fp8 mirror would have to be re-quantised in the middle of a scale period")
        if self.fp8 and self._pg is not None:
            raise KvqError("TrainEngine: param_groups / decoupled_weight_decay with fp8 forward GEMMs (fp8_forward / KVQ_FP8): the Adam "
                           "entries that write the fp8 weight mirror (kvq_adam_step_*_fp8) have no grouped form; the learning-rate "
                           "schedule options alone compose with fp8")
        if self._pg is not None:
            # the tables kvq_adam_step_grouped reads, on the device, once: one byte per 16-element block of the flat buffer, and the
            # groups' scales and decays.  Derived from the constructor's arguments: not training state.
            fl = self.flat
            blocks = param_group_blocks([(n, o) for n, (o, _, _) in fl.seg.items()], fl.n, self._pg["group_of"])
            self._pg.update(blocks_host=blocks, blocks=blocks.to(dev),
                            scale=torch.tensor([g["lr_scale"] for g in self._pg["table"]], dtype=torch.float32, device=dev),
                            wd=torch.tensor([g["weight_decay"] for g in self._pg["table"]], dtype=torch.float32, device=dev),
                            range_group={})
        self._lr_out = self._state[1:2].view(torch.float32)[0]      # the step state's lr, a view: train_step hands out copies
        self._fp8_fused = fp8_forward == "fused"
        self._fp8_all = fp8_forward in ("all", "fused")
        self._x8 = {}                      # data_ptr of a bf16 activation -> its fp8 copy, left by the producer for ONE fp8 GEMM
        # option, off by default: input-gradient GEMMs gx = gy . W of the training step on the fp8 matrix cores --
        # gy quantised to e5m2 by a delayed-scaling pass, against the byte-transposed e4m3 weight mirror (_w8t).  None: KVQ_FP8_BACKWARD
        # from the environment, as fp8_forward reads KVQ_FP8 (bench.py --fp8 measures both arms that way; unset = off; it is ignored
        # on an engine without fp8 forward GEMMs).  None is the DEFAULT: with KVQ_FP8_BACKWARD=1 in the environment every engine with
        # fp8 forward GEMMs that does not pass False takes the option, and its backward bits change; pass False to rule that out.  Needs fp8 forward GEMMs, theirs is the weight mirror: an explicit True without
        # them is refused.
        if fp8_backward is None:
            fp8_backward = self.fp8 and os.environ.get("KVQ_FP8_BACKWARD", "0") == "1"
        if fp8_backward not in (False, True):
            raise KvqError(f"TrainEngine: fp8_backward must be False, True or None (KVQ_FP8_BACKWARD), got {fp8_backward!r}")
        self.fp8_backward = bool(fp8_backward)
        if self.fp8_backward and not self.fp8:
            raise KvqError("TrainEngine: fp8_backward needs fp8 forward GEMMs (fp8_forward / KVQ_FP8): the input-gradient GEMMs read "
                           "the transposed copy of the forward's e4m3 weight mirror")
        # option, off by default: the step measures the global norm of its gradient between backward and Adam
        # (kvq_grad_sumsq_partial / kvq_grad_guard_finalize), Adam scales the gradient by min(1, max_grad_norm / (norm + 1e-6)) --
        # torch.nn.utils.clip_grad_norm_ -- and a step whose gradient is not finite stores nothing.  float("inf"): measure and
        # guard, never clip.  None: KVQ_MAX_GRAD_NORM from the environment, as fp8_backward reads KVQ_FP8_BACKWARD; unset / empty: off.
        # Off = no guard buffer, no launch added, today's Adam calls.
        self._guard = self._gn_partials = None
        if self.max_grad_norm is not None:
            self._gn_P = nnops.grad_sumsq_partials()
            self._guard = nnops.new_grad_guard(dev)
            f = self._guard[1:2].view(torch.float32)
            self._guard_out = dict(grad_norm=f[0], grad_clip_coef=f[1])      # views: train_step hands out copies
        # option, off by default: gradient accumulation.  grad_accum = A > 1: every train_step call is a
        # MICRO-step -- forward, backward, flat gradient added into an f32 accumulator (kvq_grad_accumulate) -- and every A-th call
        # also runs the optimiser on the mean of the A gradients: (loss / A).backward() A times, opt.step() once.  None:
        # KVQ_GRAD_ACCUM from the environment, as max_grad_norm reads KVQ_MAX_GRAD_NORM (unset / empty: 1).  A = 1: no buffer, no
        # launch added, today's step and graphs.  The position inside a cycle lives on the device (include/kvq.h "gradient
        # accumulation"); the dropout seeds follow its micro-step count instead of the optimiser step count, which stands still
        # inside a cycle.  (The combinations refused at the top of the constructor are each a piece of work of their own.)
        self._acc_state, self._seed_state, self._accum_host, self._grads_are_mean = None, self._state, 0, False
        if self.grad_accum > 1:
            self._acc_state = self._seed_state = nnops.new_accum_state(dev)
            for a in self.aux:
                if a["p"].requires_grad:
                    a["acc"] = torch.zeros_like(a["p"].data)
        # option, off by default: an exponential moving average of the trained weights.  weight_ema = decay
        # in (0, 1): behind Adam every optimiser step moves an f32 average of each trainable range of the master buffer and of each
        # aux parameter Adam owns (kvq_weight_ema_update; the first update stores, the decay warms up as min(decay, (1 + t) / (10 + t))),
        # and weight_ema_applied() evaluates under it.  None: KVQ_WEIGHT_EMA from the environment, as max_grad_norm reads
        # KVQ_MAX_GRAD_NORM (unset / empty: off).  Off = no buffer, no launch added, today's step and graphs.  The update count lives
        # on the device (include/kvq.h "exponential moving average of the trained weights"): a skipped step does not count.
        self._wema_state, self._wema_applied = None, False
        if self.weight_ema is not None:
            self._wema_state = nnops.new_weight_ema_state(dev)
            self._wema_out = self._wema_state[1:2].view(torch.float32)[0]      # last_decay, a view: train_step hands out copies
            for a in self.aux:
                if a["p"].requires_grad:
                    a["ema"] = torch.zeros_like(a["p"].data)
        # fp8 input-gradient GEMMs of the last training step and their weight keys in launch order: counted while the step is
        # scheduled (eagerly, or at capture -- a replay restores the counts of the graphs it replays)
        self.fp8_bwd_launches = 0
        self.fp8_bwd_sites = []
        self._bwd8_mode = None             # "calibrate" | "run" while a training step's backward is scheduled
        self._g8_index, self._g8_live, self._g8_ready, self._w8t = {}, set(), False, None
        if self.fp8:
            if self.dtype != torch.bfloat16:
                raise KvqError("TrainEngine: fp8 forward GEMMs need the bf16 compute dtype")
            self._fp8_setup()
        # Off = no idle buffer, no launch added, today's graphs.  On: usage flags + select behind the quantiser's forward launch (the
        # eager interlude of the step), apply behind the codebook's own update (_revive_apply); state on the module when it has some
        self._rv_pending = self._in_fb = False
        self.revive_keep_donors = False          # tests: keep a copy of the z the select kernel read (revive_donors)
        if self.revive_after is not None:
            vq = model.vector_quantizer
            own = getattr(vq, "revive_after", None) is None           # the option came from the environment: the state is the engine's
            self._rv_idle = torch.zeros((self.G, self.K), dtype=torch.int32, device=dev) if own else vq.code_idle
            self._rv_counter = new_revive_counter(dev) if own else vq.revive_counter
            if self._rv_idle.numel() != self.G * self.K or not self._rv_idle.is_cuda:
                raise KvqError(f"TrainEngine: code_idle {tuple(self._rv_idle.shape)} does not match {self.G} x {self.K} codes on the device")
            self._rv_used = torch.zeros((self.G, self.K), dtype=torch.int32, device=dev)
            self._rv_rows = torch.zeros((self.G, self.K, self.Dg), dtype=torch.float32, device=dev)
        model.__dict__["_kvq_engine"] = self
        self._param_versions = self._versions()
        # gradient all-reduce chunks (tail first)
        self.comm_stream = torch.cuda.Stream(device=dev) if self._dp else None
        self._avg_in_comm = self._dp and dist.get_backend(process_group) == "nccl"   # RCCL averages itself; gloo sums
        self.chunk = max(bucket_mib * (1 << 20) // torch.empty(0, dtype=self.flat.compute_dtype).element_size(), 1 << 16)     # elements per all-reduce chunk
        self._pending_hi = self._wg_done_lo = self.flat.n
        self._works, self._works_late = [], []
        self._ev_early = torch.cuda.Event() if self._dp else None
        self._time_comm = False
        self._comm_ev = []                       # (start, end) event pairs around the points where the compute stream waits for RCCL
        self._ones = torch.ones((), dtype=torch.float32, device=dev)
        self._g_recon = torch.full((), self.w_recon, dtype=torch.float32, device=dev)     # d total / d loss term: constants of the run
        self._g_vq = torch.full((), self.w_vq, dtype=torch.float32, device=dev)
        self._g_vq_ext = None                  # backward_from(): the caller's d L / d loss_vq_raw instead of the run's constant
        _load_gemm_tuning()

    # ------------------------------------------------------------------------------------------------------------
    # small helpers
    # ------------------------------------------------------------------------------------------------------------
    def __deepcopy__(self, memo):
        return None                   # copy.deepcopy(model): the copy builds its own engine on first use (engine_of)

    def __reduce__(self):
        return (type(None), ())       # torch.save(model): the engine (streams, graphs, flat mirrors) is not part of a checkpoint

    @property
    def pad_idx(self):
        """padding_idx of the word embeddings (None = no padding row): the id a packed batch files under -1 (prepare_batch)."""
        return self._pad_idx

    @property
    def step_count(self):
        """Optimiser steps applied so far (host mirror of the device step state).  With grad_accum > 1 a train_step call is a
        micro-step: this counts the calls that ran the optimiser, as the milestones and Adam's bias corrections do."""
        return self._step_host

    @step_count.setter
    def step_count(self, n):
        self._step_host = int(n)
        self._state[0] = int(n)          # lr / bias corrections are recomputed by the next kvq_step_state_advance
        if self._acc_state is not None:  # n finished cycles: the masks continue where a run of n optimiser steps would be
            self._acc_state[0] = int(n) * self.grad_accum
            self._acc_state[1] = 0
            self._accum_host, self._grads_are_mean = 0, False

    @property
    def accum_pending(self):
        """Micro-steps of the current cycle already in the accumulator (host mirror of the device's `micro`; 0 with grad_accum 1)."""
        return self._accum_host

    def reset_accumulation(self):
        """Drop a started cycle: the next train_step is the first micro-step of a new one (it stores, so what the accumulator holds
        does not matter).  The micro-step count `tick` is left alone -- the dropout masks move on."""
        if self._acc_state is not None:
            self._acc_state[1] = 0
        self._accum_host, self._grads_are_mean = 0, False

    def _lr_now(self):
        """MultiStepLR ticked once per optimiser step (Trainer.py:114-115): the s-th step (1-based) sees s-1 ticks."""
        ticks = self.step_count - 1
        k = sum(1 for m in self.milestones if ticks >= m)
        if self.lr_schedule is not None:          # warm-up / decay of kvq_step_state_advance_sched, mirrored on the host
            return self.lr * (self.gamma ** k) * lr_schedule_factor(self.step_count, *self.lr_schedule)
        return self.lr * (self.gamma ** k)

    def _site(self):
        self._site_ctr += 1
        return self._site_ctr

    # Tile choice: kvq.nnops.pick_tile / persistent_pays (a cost model over (M, N, K) fitted to tools/gemm2_probe_small.py and
    # consistent with the per-shape choices measured at 8192 rows in rounds 2 - 3, which it replaced).  KVQ_GEMM_TILE="NxK:tile;..."
    # overrides it per weight shape for A/B runs on the GPU box.
    _TILE_OVERRIDE: Dict[Tuple[int, int], str] = {}

    # ---- fp8 forward GEMMs -------------------------------------------------------------------------------------------------
    _FP8_MIN_ROWS = 8192          # output width from which fp8 + its quantisation pass beat the bf16 kernel (see __init__)

    def _fp8_setup(self):
        """One fp8 mirror of the flat bf16 shadow buffer; one quantisation segment (= one scale) per forward GEMM weight: the
        fused q|k|v block, the all-layer cross-attention k|v block, every other [out, in] matrix, the padded LM-head table."""
        fl = self.flat
        segs = {}

        def seg(key, names, rows=None):
            o0 = fl.seg[names[0]][0]
            n = sum(fl.seg[nm][1] for nm in names) if rows is None else rows * fl.seg[names[0]][2][1]
            only = os.environ.get("KVQ_FP8_ONLY")          # diagnostic: "all" restricted to weights whose name contains one of these
            if only and not any(t in key for t in only.split(",")):
                return
            if self._fp8_all or n // fl.seg[names[0]][2][1] >= self._FP8_MIN_ROWS:
                segs[key] = (o0, n)
        for i in range(self.n_enc_layers):
            pre = f"enc.{i}."
            seg(pre + "sa.q.w", [pre + "sa.q.w", pre + "sa.k.w", pre + "sa.v.w"])
            for nm in ("sa.o.w", "f1.w", "f2.w"):
                seg(pre + nm, [pre + nm])
        for i in range(self.n_dec_layers):
            pre = f"dec.{i}."
            seg(pre + "sa.q.w", [pre + "sa.q.w", pre + "sa.k.w", pre + "sa.v.w"])
            for nm in ("sa.o.w", "ca.q.w", "ca.o.w", "f1.w", "f2.w"):
                seg(pre + nm, [pre + nm])
            if not self._cakv_batched:
                seg(pre + "ca.k.w", [pre + "ca.k.w", pre + "ca.v.w"])
        if self._cakv_batched:
            seg(self._cakv_w[0], self._cakv_w)
        seg("head.t.w", ["head.t.w"])
        seg("dec.emb.word", ["dec.emb.word"], rows=self.Vp)
        keys = list(segs)
        if not keys:
            raise KvqError("TrainEngine: fp8 forward GEMMs asked for, but no weight of this model is wide enough for them to pay "
                           f"(>= {self._FP8_MIN_ROWS} rows); fp8_forward=True / \"fused\" puts every forward GEMM on fp8")
        self._w8_index = {k: i for i, k in enumerate(keys)}
        offs = [segs[k][0] for k in keys]
        ns = [segs[k][1] for k in keys]
        assert all(o % 16 == 0 and n % 16 == 0 for o, n in zip(offs, ns))
        self._w8 = torch.zeros(fl.n, dtype=torch.uint8, device=self.dev)
        self._w8_off = torch.tensor(offs, dtype=torch.int64, device=self.dev)
        self._w8_n = torch.tensor(ns, dtype=torch.int64, device=self.dev)
        self._w8_max = max(ns)
        self._w8_period = max(int(os.environ.get("KVQ_FP8_W_PERIOD", "16")), 1)
        # the Adam kernel writes the fp8 mirror itself (kvq_adam_step_dev_fp8) when the scales are not refreshed on every step:
        # span_segment[e >> 11] = the segment covering elements [2048 k, 2048 k + 2048), -1 none, -2 several things
        self._w8_in_adam = self._w8_period > 1 and os.environ.get("KVQ_FP8_ADAM", "1") != "0"
        self._w8_span = torch.from_numpy(fp8_span_table(offs, ns, fl.n)).to(self.dev)
        self._w8_amax = torch.zeros(len(keys), dtype=torch.float32, device=self.dev)
        self._w8_scale = torch.ones(len(keys), dtype=torch.float32, device=self.dev)
        self._w8_adam = (self._w8, self._w8_span, self._w8_scale, self._w8_off, self._w8_n, len(keys))   # nnops.adam_step_dev(fp8=)
        if self.fp8_backward:
            self._fp8_bwd_setup(keys, offs, ns)
        self._fp8_quantize_weights()
        # activations: one {scale, amax} pair per GEMM input of the step, in call order (delayed scaling: include/kvq.h)
        self._a8_sites = len(keys)                    # one record per fp8 GEMM = per weight key (each is used once per forward)
        st = torch.zeros((self._a8_sites, lib().kvq_fp8_state_floats()), dtype=torch.float32, device=self.dev)
        st[:, 0] = 1.0
        self._a8_state = st

    # ---- fp8 input-gradient GEMMs (option fp8_backward) ---------------------------------------------------------------------
    _FP8_BWD_HEADROOM = 4.0       # as the forward sites: scale = max(e5m2) / (4 amax of the previous step)

    def _fp8_bwd_setup(self, keys, offs, ns):
        """The sites: every weight W [M, K] with a forward fp8 segment whose input gradient gx[N, K] = gy[N, M] . W can run as the NT
        product gy8 . (W^T8)^T of the fp8 kernel -- the contraction M a multiple of 128 (the LM head's 30528 = 238.5 x 128 is not:
        it stays bf16), K a multiple of 16.  Per site: the segment of the transposed mirror _w8t (dense, [K, M]; rebuilt from _w8
        by ONE segmented transpose wherever _w8 changes) and one delayed-scaling record for gy in e5m2, scale 0 = not calibrated.
        Which of these sites the backward really visits depends on the batch (BertOutput's input gradient is folded into the
        GELU' GEMM at the shapes where that tile exists, and never comes here): the table starts with every candidate, and after
        the calibration step the per-step transpose is cut down to the sites that are live (_fp8_bwd_end)."""
        fl = self.flat
        only = os.environ.get("KVQ_FP8_BWD_ONLY")        # diagnostic: restrict the sites to weights whose name contains one of these
        sites, doff = [], 0
        for key, o, n in zip(keys, offs, ns):
            K = fl.seg[key][2][1]
            M = n // K
            if M * K != n or M % 128 or K % 16 or (only and not any(t in key for t in only.split(","))):
                continue
            sites.append((key, o, M, K, doff))
            doff += n
        if not sites:
            raise KvqError("TrainEngine: fp8_backward asked for, but no weight with an fp8 forward segment has an eligible input "
                           "gradient (contraction length a multiple of 128)" + (f"; KVQ_FP8_BWD_ONLY={only}" if only else ""))
        assert all(o % 16 == 0 and d % 16 == 0 and M % 16 == 0 and K % 16 == 0 for _, o, M, K, d in sites)
        self._g8_index = {key: i for i, (key, *_) in enumerate(sites)}
        self._w8t_seg = {key: (d, M, K) for key, _, M, K, d in sites}
        self._w8t = torch.zeros(doff, dtype=torch.uint8, device=self.dev)
        self._w8t_sites = sites
        self._fp8_transpose_table(sites)
        self._g8_state = torch.zeros((len(sites), lib().kvq_fp8_state_floats()), dtype=torch.float32, device=self.dev)

    def _fp8_transpose_table(self, sites):
        """The device tables of the per-step segmented transpose for these sites (none: no launch)."""
        t64 = lambda v: torch.tensor(v, dtype=torch.int64, device=self.dev)
        self._w8t_tab = (t64([o for _, o, _, _, _ in sites]), t64([M for _, _, M, _, _ in sites]), t64([K for _, _, _, K, _ in sites]),
                         t64([d for *_, d in sites])) if sites else None
        self._w8t_tiles = max((-(-M // 128) * -(-K // 128) for _, _, M, K, _ in sites), default=0)

    def _fp8_transpose_weights(self):
        if self._w8t_tab is not None:
            nnops.fp8_transpose_segments(self._w8, self._w8t, *self._w8t_tab, self._w8t_tiles)

    def _fp8_bwd_begin(self, compute_grads):
        """Start of a forward_backward call: what its backward does at an eligible site.  The FIRST training step of the engine
        calibrates: every input gradient runs on bf16 and each site only notes the amax of its gy (a delayed scale of 1 would flush
        gradients, whose magnitudes sit near e5m2's smallest subnormal, to zero -- nothing is quantised with a scale that does not
        come from a measured amax of that site).  It is eager (train_step defers the capture): the scales are read back after it."""
        self._bwd8_mode = None
        if not (self.fp8_backward and compute_grads):
            return
        self.fp8_bwd_launches, self.fp8_bwd_sites = 0, []
        if self._g8_ready:
            self._bwd8_mode = "run"
            return
        if self._cap is not None or torch.cuda.is_current_stream_capturing():
            raise KvqError("TrainEngine: the calibration step of fp8_backward (the first training step) cannot be captured")
        self._bwd8_mode = "calibrate"

    def _fp8_bwd_end(self):
        """End of a training step's backward: next step's gradient scales from this step's amax (kernel; captured with the step).
        After the calibration step: the sites whose amax was 0 -- a frozen branch, or a batch the site was not eligible at -- keep
        scale 0 and stay on bf16."""
        mode, self._bwd8_mode = self._bwd8_mode, None
        if mode is None:
            return
        check(lib().kvq_fp8_update_scales_fmt(self._g8_state.data_ptr(), len(self._g8_index), self._FP8_BWD_HEADROOM, FP8_E5M2, stream_ptr()),
              "kvq_fp8_update_scales_fmt")
        if mode == "calibrate":
            sc = self._g8_state[:, 0].cpu()
            self._g8_live = {k for k, i in self._g8_index.items() if float(sc[i]) > 0.0 and bool(torch.isfinite(sc[i]))}
            self._g8_ready = True
            # from here on only the live sites' weights are transposed every step (the others' segments of _w8t are never read)
            self._fp8_transpose_table([t for t in self._w8t_sites if t[0] in self._g8_live])
            if not self._g8_live:
                import sys
                print("[kvq] fp8_backward: the calibration step (the first training step) left no input-gradient site with a measured "
                      "amax -- a batch of fewer than 256 tokens, or every branch frozen; all input gradients of this engine stay on "
                      "bf16", file=sys.stderr, flush=True)

    def _dgrad_fp8(self, gy, key, out=None):
        """gx = gy . W (added to `out` when given) on the fp8 matrix cores, or None where this product stays on the bf16 kernel: the
        key has no site, gy has fewer than 256 rows or a contraction length that is no multiple of 128, strides that are not unit /
        16-byte aligned, an uncalibrated or frozen site, the calibration step (which notes gy's amax here)."""
        if self._bwd8_mode is None or key not in self._g8_index:
            return None
        if gy.dtype != torch.bfloat16 or gy.dim() != 2 or gy.shape[0] < 256 or gy.shape[1] % 128 or gy.stride(1) != 1 or gy.stride(0) % 8 \
                or gy.data_ptr() % 16:
            return None
        d, M, K = self._w8t_seg[key]
        if gy.shape[1] != M or (out is not None and (out.dtype != torch.bfloat16 or out.shape != (gy.shape[0], K) or out.stride(1) != 1
                                                     or out.stride(0) % 8 or out.data_ptr() % 16)):
            return None
        st = self._g8_state[self._g8_index[key]]
        if self._bwd8_mode == "calibrate":
            nnops.fp8_quantize_delayed(gy, st, FP8_E5M2, amax_only=True)
            return None
        if key not in self._g8_live:
            return None
        g8 = nnops.fp8_quantize_delayed(gy, st, FP8_E5M2)
        Wt8 = self._w8t[d:d + M * K].view(K, M)
        self.fp8_bwd_launches += 1
        self.fp8_bwd_sites.append(key)
        return nnops.gemm_fp8_nt(g8, Wt8, st[0:], self._w8_scale[self._w8_index[key]:], out=out, a_format=FP8_E5M2,
                                 accumulate=out is not None)

    def _a8_state_of(self, key):
        """The delayed-scaling record of the fp8 GEMM with weight `key` (its input's scale and amax partials)."""
        return self._a8_state[self._w8_index[key]]

    def _emits_fp8_for(self, key):
        """True when the kernel that produces the input of GEMM `key` should write its fp8 copy too (scope "fused")."""
        return self.fp8 and self._fp8_fused and key is not None and key in self._w8_index

    def _fp8_quantize_weights(self, in_step=False):
        """The GEMM weights of the whole model to fp8 (two passes over the bf16 shadow: amax per weight, then the conversion).
        in_step: after an optimiser step of the engine -- the amax pass (and with it the scales) runs on every
        KVQ_FP8_W_PERIOD-th step only (default 16, decided from the device step count, so that graph replay follows): between
        refreshes a weight that outgrew its amax saturates, and an Adam step moves a weight by ~lr."""
        if in_step and self._w8_period > 1:
            # (negative period: the Adam kernel has written this step's bytes, the conversion pass runs on refresh steps only)
            per = -self._w8_period if self._w8_in_adam else self._w8_period
            check(lib().kvq_fp8_quantize_segments_periodic(self.flat.shadow.data_ptr(), self._w8_off.data_ptr(), self._w8_n.data_ptr(),
                                                           len(self._w8_index), self._w8_max, self._w8.data_ptr(), self._w8_amax.data_ptr(),
                                                           self._w8_scale.data_ptr(), self._state.data_ptr(), per, stream_ptr()),
                  "kvq_fp8_quantize_segments_periodic")
        else:
            check(lib().kvq_fp8_quantize_segments(self.flat.shadow.data_ptr(), self._w8_off.data_ptr(), self._w8_n.data_ptr(),
                                                  len(self._w8_index), self._w8_max, self._w8.data_ptr(), self._w8_amax.data_ptr(),
                                                  self._w8_scale.data_ptr(), stream_ptr()), "kvq_fp8_quantize_segments")
        if self._w8t is not None:          # the mirror changed (here, or in the Adam kernel just before): so does its transposed copy
            self._fp8_transpose_weights()

    def _linear_fp8(self, x, W, b, key):
        si = self._w8_index[key]
        o = self.flat.seg[key][0]
        W8 = self._w8[o:o + W.numel()].view(W.shape)
        st = self._a8_state[si]
        x8 = self._fp8_input(x, st, key)
        return nnops.gemm_fp8_nt(x8, W8, st[0:], self._w8_scale[si:], bias=b)

    def _fp8_input(self, x, st, key):
        """The fp8 copy of activation x for the GEMM with weight `key` (record `st`): the one the producer of x left for exactly
        this GEMM (scope "fused"), or a quantisation pass."""
        x8 = self._x8.pop((x.data_ptr(), key), None)
        if x8 is not None and tuple(x8.shape) == tuple(x.shape):
            return x8
        x8 = torch.empty(x.shape, dtype=torch.uint8, device=self.dev)
        check(lib().kvq_fp8_quantize_delayed(x.data_ptr(), x.shape[0], x.shape[1], x.stride(0), x8.data_ptr(), st.data_ptr(), stream_ptr()),
              "kvq_fp8_quantize_delayed")
        return x8

    def _linear(self, x, wname, bname, fused=None, Wb=None, key=None):
        if Wb is not None:
            W, b = Wb
        else:
            W = self.flat.fused(fused[0], self.flat.shadow) if fused else self.flat.w(wname)
            b = self.flat.fused(fused[1], self.flat.shadow) if fused else self.flat.w(bname)
            key = fused[0][0] if fused else wname
        if self.fp8 and key in self._w8_index and x.shape[0] >= 256 and W.shape[1] % 128 == 0 and x.stride(1) == 1:
            return self._linear_fp8(x, W, b, key)
        return self._gemm(x, W, "nt", bias=b)

    def _gemm(self, a, b, layout, bias=None, out=None, accumulate=False, tile=None):
        """op(a) . op(b) (+ bias) (accumulated into out).  bf16: libkvq.so, always (nnops.gemm: MFMA kernel or the any-shape one).
        f32 (the checker engine) and KVQ_OWN_GEMM=0 (A/B against the vendor library): torch."""
        if self._own_fwd and self.dtype == torch.bfloat16:
            M, N, K = nnops._gemm_dims(a, b, layout)
            wshape = (N, K) if layout == "nt" else ((K, N) if layout == "nn" else (M, N))
            return nnops.gemm(a, b, layout, bias=bias, out=out, accumulate=accumulate, tile=self._TILE_OVERRIDE.get(wshape, tile))
        A = a.t() if layout == "tn" else a
        Bm = b.t() if layout == "nt" else b
        if out is not None and accumulate:
            return out.addmm_(A, Bm)
        if out is not None:
            return torch.mm(A, Bm, out=out) if bias is None else torch.addmm(bias, A, Bm, out=out)
        return torch.addmm(bias, A, Bm) if bias is not None else torch.mm(A, Bm)

    def _epilogue_tile(self, M, N, K):
        """Tile of the fused-activation GEMMs (they exist for 256 x 192 and 128 x 256), or None when the plain GEMM on its best
        tile + the separate activation kernel (one pass over [M, N]: ~3 us + 4 bytes per element at ~3 TB/s) is modelled cheaper --
        outputs too small to give half the CUs one of the large tiles."""
        if not (self._own_fwd and self.dtype == torch.bfloat16):
            return None
        t = nnops.pick_tile(M, N, K, candidates=("256x192", "128x256"))
        plain = nnops.tile_cost_us(nnops.pick_tile(M, N, K), M, N, K) + 3.0 + M * N * 4 / 3e6
        return nnops.TILE_NAMES[t] if nnops.tile_cost_us(t, M, N, K) <= plain else None

    def _dense_residual_ln(self, a, wname, bname, resid, gname, betaname, eps, p_drop, site, next_key=None):
        """LayerNorm(dropout(a . W^T + b) + resid) of a BertSelfOutput / BertOutput block (modeling_bert.py:282-296, 339-352):
        (out, pre, mean, rstd) as nnops.ln_fwd returns them.  bf16 engine: the dense layer's epilogue draws the dropout mask, adds
        the residual and stores `pre` (nnops.gemm_dropres -- bit for bit the `pre` of the two-kernel form), then LayerNorm alone."""
        fl = self.flat
        W, b = fl.w(wname), fl.w(bname)
        gamma, beta = fl.w32(gname), fl.w32(betaname)
        if (self._fuse_dropres == "1" or (self._fuse_dropres == "eval" and p_drop == 0.0)) and self._own_fwd \
                and self.dtype == torch.bfloat16 \
                and not (self.fp8 and wname in self._w8_index) and a.is_contiguous() and resid.is_contiguous() \
                and nnops.gemm_mfma_ok(a, W, None, "nt", b):
            pre = nnops.gemm_dropres(a, W, b, resid, p_drop, self._step_seed, site)
            out, _, mean, rstd = nnops.ln_fwd(pre, None, gamma, beta, eps, 0.0, 0, 0, save_pre=False)
            return out, pre, mean, rstd
        y = self._linear(a, wname, bname)
        if self._emits_fp8_for(next_key):             # next_key: the GEMM that reads this block's output
            out, pre, mean, rstd, out8 = nnops.ln_fwd_fp8(y, resid, gamma, beta, eps, p_drop, self._step_seed, site, self._a8_state_of(next_key))
            self._x8[(out.data_ptr(), next_key)] = out8
            return out, pre, mean, rstd
        return nnops.ln_fwd(y, resid, gamma, beta, eps, p_drop, self._step_seed, site)

    def _linear_gelu(self, x, wname, bname, next_key=None):
        """(h, gelu(h)), h = x . W^T + b: one kernel where the own GEMM carries the activation in its epilogue."""
        W, b = self.flat.w(wname), self.flat.w(bname)
        on_fp8 = self.fp8 and wname in self._w8_index         # (fp8 "all": the fp8 GEMM has no activation epilogue)
        if on_fp8 and self._fp8_fused and x.shape[0] >= 256 and W.shape[1] % 128 == 0 and x.is_contiguous():
            # scope "fused": BertIntermediate on the fp8 matrix cores WITH the GELU epilogue, which also leaves the fp8 copy of
            # gelu(h) for BertOutput.dense (next_key)
            si = self._w8_index[wname]
            o = self.flat.seg[wname][0]
            W8 = self._w8[o:o + W.numel()].view(W.shape)
            st = self._a8_state[si]
            x8 = self._fp8_input(x, st, wname)
            if self._emits_fp8_for(next_key):
                h, a, a8 = nnops.gemm_fp8_nt_gelu(x8, W8, st[0:], self._w8_scale[si:], b, state_out=self._a8_state_of(next_key))
                self._x8[(a.data_ptr(), next_key)] = a8
                return h, a
            return nnops.gemm_fp8_nt_gelu(x8, W8, st[0:], self._w8_scale[si:], b)
        tile = None if on_fp8 else self._epilogue_tile(x.shape[0], W.shape[0], W.shape[1])
        if tile is not None and x.is_contiguous() and nnops.gemm_mfma_ok(x, W, None, "nt", b):
            return nnops.gemm_gelu(x, W, b, tile=tile)
        h = self._linear(x, wname, bname)
        return h, nnops.gelu_fwd(h)

    # ------------------------------------------------------------------------------------------------------------
    # deferred small reductions: a layer's split-K slab sums and LayerNorm / bias partial sums go out as ONE launch
    # (kvq_reduce_batch) instead of 8-14 launch-latency-bound kernels; _flush_reductions() runs before anything reads them
    # ------------------------------------------------------------------------------------------------------------
    def _defer(self, src, dst, count, cols, ld, src_offset=0):
        self._red_items.append(nnops.reduce_item(src, dst, count, cols, ld, src_offset=src_offset))
        self._red_keep.append(src)            # the partials must outlive the launch

    _WG_MAX = 16                                          # problems per grouped launch (csrc/kvq_gemm2.hip MAX_PROBLEMS)

    # ------------------------------------------------------------------------------------------------------------
    # weight-gradient queue.  A 256 x 256 TN tile over the whole token contraction keeps its CU for ~195 us whatever runs
    # beside it, so a launch of up to one tile per CU costs one round of 210 - 225 us whether it holds 135, 216 or 255 tiles:
    # the queue exists to make every round a full one.
    #   * layers are held until two are there (_flush_wgrads): 216 (encoder) / 252 (decoder) tiles of 256 x 256;
    #   * packed schedule (_wg_pack: one process, KVQ_WG_PACK != 0) --
    #       - an output of between one and two rounds (the LM head, [30528, 768]) is one launch on two tile shapes
    #         (nnops.gemm tile "mixed": the rows that fill the CUs once on 256 x 256 tiles, the rest on 128 x 256 tiles);
    #       - weight gradients that belong to no layer pair are not queued but WAIT (_wgrad_fill) for the CUs a grouped
    #         launch leaves idle, and are taken in whole units of rows: head.t.w in 256-row slices (3 tiles; a decoder pair
    #         leaves 4 CUs), the all-layer cross-K/V gradient in per-layer slices (18 tiles; an encoder pair leaves 40).
    #         So head.t.w never breaks the pairing -- (11, 10) .. (1, 0) in both stacks -- and cross-K/V has no round of its own;
    #     everything is derived from tile counts and the CU count: what does not fit (other widths, frozen stacks, fewer
    #     layers) is launched as before, and what nothing took goes out with the forced flush that ends backward;
    #   * with a process group the schedule is the unpacked one, exactly: _wg_done_lo takes gradients to become final in
    #     buffer order.
    # Each output element comes from the same tile code, k order and accumulation in either schedule: bit-identical.
    # ------------------------------------------------------------------------------------------------------------
    def _wg_reset(self):
        self._wg_items, self._wg_keep = [], []
        self._wg_fill = []                    # packed: [gy, x, out, unit rows, next row] waiting for launches with idle CUs

    @staticmethod
    def _wg_tiles(items, bm, bn):
        return sum(-(-p.M // bm) * -(-p.N // bn) for p in items)

    def _wgrad_fill(self, gy, x, out, unit):
        """Packed schedule: gW = gy^T x without a launch of its own -- grouped launches that leave CUs idle take it in
        pieces of whole `unit` rows (a multiple of 256: whole tile rows); gy and x stay alive until the last piece is taken.
        Otherwise _wgrad."""
        if self._wg_pack and unit % 256 == 0 and out.shape[0] % unit == 0 and gy.shape[0] % 64 == 0 \
                and nnops.gemm_mfma_ok(gy, x, out, "tn"):
            self._wg_fill.append([gy, x, out, unit, 0])
            return
        self._wgrad(gy, x, out)

    def _take_fill(self, idle, bm, room):
        """At most `room` problems whose bm x 256 tiles fit `idle` CUs: the largest units first, the small ones fill the gaps."""
        taken = []
        for f in sorted(self._wg_fill, key=lambda f: -(-(-f[3] // bm) * -(-f[2].shape[1] // 256))):
            gy, x, out, unit, r0 = f
            per_unit = -(-unit // bm) * -(-out.shape[1] // 256)
            k = min(idle // per_unit, (out.shape[0] - r0) // unit) if len(taken) < room else 0
            if k > 0:
                r1 = r0 + k * unit
                taken.append(nnops.gemm_problem(gy[:, r0:r1], x, out[r0:r1], "tn"))
                f[4], idle = r1, idle - k * per_unit
        self._wg_fill = [f for f in self._wg_fill if f[4] < f[2].shape[0]]
        return taken

    def _launch_group(self, items, fill=True):
        """items as grouped launches on the tile their count asks for; a launch with idle CUs takes waiting weight gradients."""
        t256 = self._wg_tiles(items, 256, 256)
        tile = "256x256" if self._wg_tiles(items, 128, 256) > 256 and t256 <= 320 else "128x256"
        if fill and self._wg_fill and len(items) < self._WG_MAX:
            bm = 256 if tile == "256x256" else 128
            items = items + self._take_fill(self._n_cu - self._wg_tiles(items, bm, 256), bm, self._WG_MAX - len(items))
        for i in range(0, len(items), self._WG_MAX):
            nnops.gemm_grouped(items[i:i + self._WG_MAX], "tn", tile)

    def _flush_wgrads(self, force=True):
        """The weight gradients queued so far as grouped launches, written straight into the flat bf16 gradient buffer, each
        tile contracting over all tokens (no split-K).  The kernel's rate is set by bytes staged per flop (the L2 -> LDS fill
        is the limit), so the 256 x 256 tile is the fast one -- but one BERT layer is only 108-126 of them.  The
        queue is therefore held (force=False) until TWO layers' worth is there: 216-252 tiles = one round of the 256 CUs.
        Packed schedule: the launch takes waiting weight gradients up to the CU count, and a forced flush launches what
        nothing took, a round at a time.  Returns True when no layer is left queued."""
        items = self._wg_items
        if items:
            t256 = self._wg_tiles(items, 256, 256)
            if not force and len(items) <= self._WG_MAX // 2 and 2 * t256 <= 256:
                return False                               # another layer like this one still fits the same round
            self._launch_group(items)
            self._wg_items, self._wg_keep = [], []
        while force and self._wg_fill:
            rest = self._take_fill(self._n_cu, 256, self._WG_MAX)
            if not rest:                                   # (a unit larger than the chip: whole, as _wgrad would have queued it)
                rest = [nnops.gemm_problem(gy[:, r0:], x, out[r0:], "tn") for gy, x, out, _, r0 in self._wg_fill]
                self._wg_fill = []
            self._launch_group(rest, fill=False)
        return True

    def _flush_reductions(self, force=True):
        """Launch the queued batched reductions and (see _flush_wgrads) the queued weight gradients; True if none stay queued."""
        if not self._flush_wgrads(force):
            return False                       # ... and the small sums wait with them: one launch per two layers as well
        if self._red_items:
            nnops.reduce_batch(self._red_items)       # (round 5: on a side stream, joined with the weight gradients, the step was
                                                      #  0.5 ms SLOWER -- profiles/r05_gemm_ceiling.md)
        self._red_items, self._red_keep = [], []
        return True

    def _defer_colsum(self, x, dst, cols=None):
        part = nnops.colsum_partial(x, cols)
        self._defer(part, dst, part.shape[0], part.shape[1], part.shape[1])

    def _ln_bwd(self, g_out, pre, mean, rstd, gamma, p_drop, seed, site, g_gamma, g_beta, g_bias_prev=None, need_g_resid=True):
        """LayerNorm backward; the gamma / beta / previous-dense-bias gradients are queued as deferred reductions."""
        g_y, g_resid, part = nnops.ln_bwd_partial(g_out, pre, mean, rstd, gamma, p_drop, seed, site, need_g_resid=need_g_resid,
                                                  want_dbias=g_bias_prev is not None)
        H = g_out.shape[1]
        runs = []                                            # [column offset in part, dst, cols]: adjacent targets merge
        for off, dst in ((0, g_bias_prev), (H, g_gamma), (2 * H, g_beta)):
            if dst is None:
                continue
            if runs and runs[-1][0] + runs[-1][2] == off and \
                    runs[-1][1].data_ptr() + runs[-1][2] * dst.element_size() == dst.data_ptr() and runs[-1][1].dtype == dst.dtype:
                runs[-1][2] += H
            else:
                runs.append([off, dst, H])
        for off, dst, cols in runs:
            self._defer(part, dst, part.shape[0], cols, 3 * H, src_offset=off)
        return g_y, g_resid

    def _wgrad(self, gy, x, out):
        """gW = gy^T x.  bf16: a launch of its own when the output alone fills half the CUs with 256 x 256 tiles (the LM head /
        all-layer cross-K/V weight gradients), else queued for the layer's grouped launch; both contract over ALL tokens per tile (no split-K).
        A token count that is not a multiple of 64 (the MFMA kernel's k-tile: 100 sentences x 12 tokens, the last batch of an
        epoch) is zero-padded first -- zero rows of gy / x add nothing -- so that the step stays on the MFMA kernels; only what
        cannot be padded in 16-byte pieces goes to the any-shape kernel."""
        Ntok, M = gy.shape
        N = x.shape[1]
        if self._own_wgrad and Ntok % 64 != 0 and Ntok > 64:
            padded = nnops.tn_operands_k64(gy, x)
            if padded is not None:
                gy, x = padded
        if self._own_wgrad and nnops.gemm_mfma_ok(gy, x, out, "tn"):
            if -(-M // 256) * -(-N // 256) >= 128:
                # packed schedule: between one and two rounds of 256 x 256 tiles -> one full round of them + a shorter one of 128 x 256
                mixed = self._wg_pack and nnops.mixed_split(M, N, self._n_cu) > 0
                self._gemm(gy, x, "tn", out=out, tile="mixed" if mixed else None)
            else:
                self._wg_items.append(nnops.gemm_problem(gy, x, out, "tn"))
                self._wg_keep += [gy, x]                       # alive until the grouped launch
            return
        self._gemm(gy, x, "tn", out=out)

    def _linear_bwd(self, gy, x, wnames, bnames, need_gx=True, gx_accum=None, bias_done=False, fill_unit=None):
        """Weight / bias gradients straight into the flat gradient buffer; returns gx (or accumulates into gx_accum).
        fill_unit: a layer outside the stacks -- its weight gradient waits for idle CUs (_wgrad_fill) in slices of that many rows."""
        fl = self.flat
        if len(wnames) == 1:
            W, gW, gb = fl.w(wnames[0]), fl.g(wnames[0]), fl.g(bnames[0])
        else:
            W, gW, gb = fl.fused(wnames, fl.shadow), fl.fused(wnames, fl.grad), fl.fused(bnames, fl.grad)
        if fl.trainable[wnames[0]]:
            if fill_unit:
                self._wgrad_fill(gy, x, gW, fill_unit)
            else:
                self._wgrad(gy, x, gW)
        if fl.trainable[bnames[0]] and not bias_done:     # bias_done: the LayerNorm backward kernel already produced it
            self._defer_colsum(gy, gb)
        if not need_gx and gx_accum is None:
            return None
        gx = self._dgrad_fp8(gy, wnames[0], out=gx_accum)         # (the key of the weight's fp8 segment, as in _linear)
        if gx is not None:
            return gx
        if gx_accum is not None:
            return self._gemm(gy, W, "nn", out=gx_accum, accumulate=True)
        return self._gemm(gy, W, "nn")

    def _dgrad(self, gy, W, key=None):
        """gx = gy . W for a gradient that is not paired with a weight / bias gradient here (LM head, batched cross-K/V)."""
        gx = self._dgrad_fp8(gy, key) if key is not None else None
        return gx if gx is not None else self._gemm(gy, W, "nn")

    # ------------------------------------------------------------------------------------------------------------
    # blocks: forward returns (output, saved); backward consumes saved
    # ------------------------------------------------------------------------------------------------------------
    def _emb_fwd(self, prefix, cfg, ids, training, word_rows=None):
        """BertEmbeddings (modeling_bert.py:53-110) as ONE kernel: gather + position / type rows + LayerNorm + dropout."""
        fl = self.flat
        B, S = ids.shape
        word = fl.w(prefix + "word", rows=word_rows) if word_rows else fl.w(prefix + "word")
        p = cfg.hidden_dropout_prob if training else 0.0
        keep = (p, self._site()) if p > 0 else None               # the mask is regenerated in backward from (seed, site)
        out, pre, mean, rstd = nnops.embed_ln_fwd(ids.reshape(-1), word, fl.w(prefix + "pos"), fl.w(prefix + "type")[0],
                                                  fl.w32(prefix + "ln.w"), fl.w32(prefix + "ln.b"), cfg.layer_norm_eps, S,
                                                  p, self._step_seed, keep[1] if keep else 0)
        return out, (ids, pre, mean, rstd, keep)

    def _emb_bwd(self, prefix, g, saved, tied_accumulate=False):
        fl = self.flat
        ids, pre, mean, rstd, keep = saved
        B, S = ids.shape
        tr = fl.trainable
        zeroed = False                                        # position / type tables already zeroed together with the word table
        # dropout(LayerNorm(x)): the mask applies to the incoming gradient, inside the LayerNorm backward kernel
        g_y, part = nnops.ln_dropout_bwd_partial(g, pre, mean, rstd, fl.w32(prefix + "ln.w"), keep[0] if keep else 0.0,
                                                 self._step_seed, keep[1] if keep else 0)
        g_pt = g_y                                            # the sum's gradient reaches the word, position and type rows alike
        Hn = g.shape[1]
        gg, gb = (fl.g(prefix + "ln.w") if tr[prefix + "ln.w"] else None), (fl.g(prefix + "ln.b") if tr[prefix + "ln.b"] else None)
        if gg is not None and gb is not None and gg.data_ptr() + Hn * gg.element_size() == gb.data_ptr():
            self._defer(part, fl.fused([prefix + "ln.w", prefix + "ln.b"], fl.grad), part.shape[0], 2 * Hn, 3 * Hn, src_offset=Hn)
        else:
            if gg is not None:
                self._defer(part, gg, part.shape[0], Hn, 3 * Hn, src_offset=Hn)
            if gb is not None:
                self._defer(part, gb, part.shape[0], Hn, 3 * Hn, src_offset=2 * Hn)
        if tr[prefix + "word"]:
            o, n, shape = fl.seg[prefix + "word"]
            gw = fl.grad[o:o + n].view(shape)
            if g_y.shape[1] % 4 == 0 and g_y.shape[1] <= 1024:
                # deterministic segmented sum over the tokens sorted by id: the order is a property of the BATCH, prepared once
                # where the batch is built (prepare_batch: dsentences.token_cache / the trainer), not inside the replayed step
                srt = self._sorted[prefix]
                if isinstance(srt, str):                  # the decoder reads the encoder's ids: one sort serves both tables
                    if self._sorted[srt] is None:
                        self._sorted[srt] = self.prepare_batch(ids)
                    srt = self._sorted[srt]
                elif srt is None:
                    srt = self._sorted[prefix] = self.prepare_batch(ids)
                # the tables are zeroed by ONE launch (word unless it accumulates into the LM-head gradient, position, token type)
                zero = [None if tied_accumulate else gw, fl.g(prefix + "pos") if tr[prefix + "pos"] else None,
                        fl.g(prefix + "type") if tr[prefix + "type"] else None]
                if all(t is None or (t.data_ptr() % 16 == 0 and (t.numel() * t.element_size()) % 16 == 0) for t in zero):
                    nnops.zero_ranges(zero)
                    zeroed = True
                elif not tied_accumulate:
                    gw.zero_()
                nnops.embed_grad(g_y, srt[1], srt[0], gw, accumulate=tied_accumulate)
            else:
                acc = torch.zeros(shape, dtype=torch.float32, device=self.dev)
                acc.index_add_(0, ids.reshape(-1), g_y.float())
                if self._pad_idx is not None:
                    acc[self._pad_idx] = 0
                if tied_accumulate:
                    gw.add_(acc.to(gw.dtype))          # LM-head weight gradient is already in there
                else:
                    gw.copy_(acc)
        # position rows get the sum over sentences, token-type row 0 the sum over all tokens: two column sums of g_pt seen as
        # [B, S*H] and [N, H], finished by the layer's batched reduction (rows that are not looked up keep a zero gradient)
        Hh = g_pt.shape[1]
        if tr[prefix + "pos"]:
            gp = fl.g(prefix + "pos")
            if not zeroed:
                gp.zero_()
            part = nnops.colsum_partial(g_pt.view(B, S * Hh))
            self._defer(part, gp[:S], part.shape[0], S * Hh, S * Hh)
        if tr[prefix + "type"]:
            gt = fl.g(prefix + "type")
            if not zeroed:
                gt.zero_()
            part = nnops.colsum_partial(g_pt)
            self._defer(part, gt[0], part.shape[0], Hh, Hh)

    def _attn_block_fwd(self, pre, x, kv_src, mask, causal, cfg, training, B, Sq, Sk, kv_pre=None, next_key=None):
        """self-attention (kv_src is None) or cross-attention on kv_src (kv_pre: its already projected [N, 2H] keys | values,
        a column slice of the all-layer projection); returns LN(dropout(dense(ctx)) + x)."""
        fl, H, nh = self.flat, self.H, self.nh
        p_attn = cfg.attention_probs_dropout_prob if training else 0.0
        p_hid = cfg.hidden_dropout_prob if training else 0.0
        site_a, site_o = self._site(), self._site()
        if kv_src is None:
            qkv = self._linear(x, None, None, fused=([pre + "q.w", pre + "k.w", pre + "v.w"], [pre + "q.b", pre + "k.b", pre + "v.b"]))
            q, k, v = qkv[:, :H], qkv[:, H:2 * H], qkv[:, 2 * H:]
            kvbuf = None
        else:
            qkv = self._linear(x, pre + "q.w", pre + "q.b")
            kvbuf = kv_pre if kv_pre is not None else \
                self._linear(kv_src, None, None, fused=([pre + "k.w", pre + "v.w"], [pre + "k.b", pre + "v.b"]))
            q, k, v = qkv, kvbuf[:, :H], kvbuf[:, H:]
        if self._emits_fp8_for(pre + "o.w") and q.dtype == torch.bfloat16 and nnops.attn_fwd_fp8_ok(Sq, Sk):
            ctx, lse, ctx8 = nnops.attn_fwd_fp8(q, k, v, mask, B, nh, Sq, Sk, causal, p_attn, self._step_seed, site_a,
                                                self._a8_state_of(pre + "o.w"))
            self._x8[(ctx.data_ptr(), pre + "o.w")] = ctx8
        else:
            ctx, lse = nnops.attn_fwd(q, k, v, mask, B, nh, Sq, Sk, causal, p_attn, self._step_seed, site_a)
        if self._maps is not None:
            self._maps_emit(pre, q, k, v, mask, causal, B, Sq, Sk, lse)
        out, lnpre, mean, rstd = self._dense_residual_ln(ctx, pre + "o.w", pre + "o.b", x, pre + "ln.w", pre + "ln.b", cfg.layer_norm_eps,
                                                         p_hid, site_o, next_key=next_key)
        # (lse: only the kernels above 32 tokens work from the saved log-sum-exp)
        return out, (x, kv_src, qkv, kvbuf, ctx, lnpre, mean, rstd, mask, causal, p_attn, p_hid, site_a, site_o, B, Sq, Sk,
                     lse if max(Sq, Sk) > 32 else None)

    def _attn_block_bwd(self, pre, g_out, saved, g_kv_src=None, g_kv_out=None, pb_kv_out=None):
        """returns g_x; for cross-attention accumulates the gradient of kv_src into g_kv_src -- or, in the batched layout, only
        leaves g_kv (and its bias partial rows) in the given column slices for the all-layer GEMMs after the decoder loop."""
        fl, H, nh = self.flat, self.H, self.nh
        x, kv_src, qkv, kvbuf, ctx, lnpre, mean, rstd, mask, causal, p_attn, p_hid, site_a, site_o, B, Sq, Sk, lse = saved
        long_kw = dict(ctx=ctx, lse=lse) if lse is not None else {}
        tr = fl.trainable
        g_ao, g_x = self._ln_bwd(g_out, lnpre, mean, rstd, fl.w32(pre + "ln.w"), p_hid, self._step_seed, site_o,
                                 g_gamma=fl.g(pre + "ln.w") if tr[pre + "ln.w"] else None,
                                 g_beta=fl.g(pre + "ln.b") if tr[pre + "ln.b"] else None,
                                 g_bias_prev=fl.g(pre + "o.b") if tr[pre + "o.b"] else None)
        g_ctx = self._linear_bwd(g_ao, ctx, [pre + "o.w"], [pre + "o.b"], bias_done=True)
        # the attention backward kernel also emits the per-sentence column sums of g_q / g_k / g_v: the q/k/v bias gradients
        # are then one deferred reduction over B rows instead of a second pass over the [N, 3H] gradient
        g_qkv = torch.empty_like(qkv)
        want_b = tr[pre + "q.b"]
        if kv_src is None:
            q, k, v = qkv[:, :H], qkv[:, H:2 * H], qkv[:, 2 * H:]
            pb = torch.empty((B, 3 * H), dtype=torch.float32, device=self.dev) if want_b else None
            nnops.attn_bwd(q, k, v, mask, g_ctx, B, nh, Sq, Sk, causal, p_attn, self._step_seed, site_a,
                           g_qkv[:, :H], g_qkv[:, H:2 * H], g_qkv[:, 2 * H:],
                           *((pb[:, :H], pb[:, H:2 * H], pb[:, 2 * H:]) if want_b else ()), **long_kw)
            if want_b:
                self._defer(pb, fl.fused([pre + "q.b", pre + "k.b", pre + "v.b"], fl.grad), B, 3 * H, 3 * H)
            self._linear_bwd(g_qkv, x, [pre + "q.w", pre + "k.w", pre + "v.w"], [pre + "q.b", pre + "k.b", pre + "v.b"], gx_accum=g_x,
                             bias_done=want_b)
        else:
            batched = g_kv_out is not None
            g_kv = g_kv_out if batched else torch.empty_like(kvbuf)
            pbq = torch.empty((B, H), dtype=torch.float32, device=self.dev) if want_b else None
            want_bkv = tr[pre + "k.b"]
            pbkv = (pb_kv_out if batched else torch.empty((B, 2 * H), dtype=torch.float32, device=self.dev)) if want_bkv else None
            nnops.attn_bwd(qkv, kvbuf[:, :H], kvbuf[:, H:], mask, g_ctx, B, nh, Sq, Sk, causal, p_attn, self._step_seed, site_a,
                           g_qkv, g_kv[:, :H], g_kv[:, H:], pbq, pbkv[:, :H] if want_bkv else None, pbkv[:, H:] if want_bkv else None,
                           **long_kw)
            if want_b:
                self._defer(pbq, fl.g(pre + "q.b"), B, H, H)
            self._linear_bwd(g_qkv, x, [pre + "q.w"], [pre + "q.b"], gx_accum=g_x, bias_done=want_b)
            if not batched:
                if want_bkv:
                    self._defer(pbkv, fl.fused([pre + "k.b", pre + "v.b"], fl.grad), B, 2 * H, 2 * H)
                self._linear_bwd(g_kv, kv_src, [pre + "k.w", pre + "v.w"], [pre + "k.b", pre + "v.b"], gx_accum=g_kv_src, bias_done=want_bkv)
        return g_x

    def _ffn_fwd(self, pre, x, cfg, training, next_key=None):
        fl = self.flat
        p_hid = cfg.hidden_dropout_prob if training else 0.0
        site = self._site()
        h, a = self._linear_gelu(x, pre + "f1.w", pre + "f1.b", next_key=pre + "f2.w")
        out, lnpre, mean, rstd = self._dense_residual_ln(a, pre + "f2.w", pre + "f2.b", x, pre + "ln2.w", pre + "ln2.b", cfg.layer_norm_eps,
                                                         p_hid, site, next_key=next_key)
        return out, (x, h, a, lnpre, mean, rstd, p_hid, site)

    def _ffn_bwd(self, pre, g_out, saved):
        fl = self.flat
        x, h, a, lnpre, mean, rstd, p_hid, site = saved
        tr = fl.trainable
        g_f, g_x = self._ln_bwd(g_out, lnpre, mean, rstd, fl.w32(pre + "ln2.w"), p_hid, self._step_seed, site,
                                g_gamma=fl.g(pre + "ln2.w") if tr[pre + "ln2.w"] else None,
                                g_beta=fl.g(pre + "ln2.b") if tr[pre + "ln2.b"] else None,
                                g_bias_prev=fl.g(pre + "f2.b") if tr[pre + "f2.b"] else None)
        W2 = fl.w(pre + "f2.w")
        tile = self._epilogue_tile(g_f.shape[0], W2.shape[1], W2.shape[0])
        if tile is not None and g_f.is_contiguous() and h.is_contiguous() and nnops.gemm_mfma_ok(g_f, W2, None, "nn"):
            # input gradient of f2, the activation's derivative and the f1-bias partial sums in ONE kernel
            self._linear_bwd(g_f, a, [pre + "f2.w"], [pre + "f2.b"], need_gx=False, bias_done=True)      # queues the f2 weight gradient
            g_h, pb = nnops.gemm_dgelu(g_f, W2, h, tile=tile)
            if tr[pre + "f1.b"]:
                self._defer(pb, fl.g(pre + "f1.b"), pb.shape[0], pb.shape[1], pb.shape[1])
            self._linear_bwd(g_h, x, [pre + "f1.w"], [pre + "f1.b"], gx_accum=g_x, bias_done=True)
            return g_x
        g_a = self._linear_bwd(g_f, a, [pre + "f2.w"], [pre + "f2.b"], bias_done=True)
        if tr[pre + "f1.b"] and h.is_contiguous() and h.shape[1] % 8 == 0:
            g_h, pb = nnops.gelu_bwd_bias(h, g_a, out=g_a)           # bias gradient partials come out of the same pass
            self._defer(pb, fl.g(pre + "f1.b"), pb.shape[0], pb.shape[1], pb.shape[1])
            self._linear_bwd(g_h, x, [pre + "f1.w"], [pre + "f1.b"], gx_accum=g_x, bias_done=True)
        else:
            g_h = nnops.gelu_bwd(h, g_a, out=g_a)
            self._linear_bwd(g_h, x, [pre + "f1.w"], [pre + "f1.b"], gx_accum=g_x)
        return g_x

    # ------------------------------------------------------------------------------------------------------------
    # gradient exchange (multi-GPU): all-reduce finished tail chunks of the flat gradient buffer while backward runs
    # ------------------------------------------------------------------------------------------------------------
    def _grads_done_down_to(self, name, partial=False):
        """Every gradient located at or after segment `name` is final (once the queued reductions have been launched).
        `partial`: also send the incomplete chunk above `name` (used before the last, late part of backward)."""
        lo = self.flat.seg[name][0]
        if not self._flush_reductions(force=partial):
            lo = self._wg_done_lo                          # weight gradients of this layer still queued: final only above there
        else:
            self._wg_done_lo = lo
        if not self._dp:
            return
        ranges = []
        while self._pending_hi - self.chunk >= lo:
            ranges.append((self._pending_hi - self.chunk, self._pending_hi))
            self._pending_hi -= self.chunk
        if partial and self._pending_hi > lo:
            ranges.append((lo, self._pending_hi))
            self._pending_hi = lo
        if ranges:                               # ONE eager interlude for all chunks that became final here (no empty graphs between)
            grad = self.flat.grad
            self._eager(lambda: [self._all_reduce_avg(grad[a:b]) for a, b in ranges])

    def _all_reduce_avg(self, t, late=False):
        works = self._works_late if late else self._works
        self.comm_stream.wait_stream(torch.cuda.current_stream(self.dev))
        with torch.cuda.stream(self.comm_stream):
            if self._avg_in_comm:
                works.append((dist.all_reduce(t, op=dist.ReduceOp.AVG, group=self.group, async_op=True), None))
            else:
                works.append((dist.all_reduce(t, op=dist.ReduceOp.SUM, group=self.group, async_op=True), t))

    def _eager(self, fn):
        """Run fn now; while a step is being captured it also becomes an eager launch between two graphs of the replay."""
        if self._cap is not None:
            self._cap.interlude(fn)
        else:
            fn()

    def _settle(self, works):
        """On the side stream: wait for these collectives (and finish the average where the backend only sums)."""
        with torch.cuda.stream(self.comm_stream):     # work.wait() orders the CURRENT stream behind the collective's result:
            for w, t in works:                        # the side stream must be the one that waits before it divides
                w.wait()
                if t is not None:
                    t.div_(self.world)
        works.clear()

    def _exchange_head(self, cut):
        """End of backward.  Everything above `cut` was sent while backward ran: settle it and let the optimiser start on
        that part; the head of the buffer [0, cut) -- the embedding gradients, final only now -- and the codebook gradient
        go out behind it and are waited for by _exchange_tail(), i.e. their all-reduce overlaps with Adam on the rest."""
        self._settle(self._works)
        self._ev_early.record(self.comm_stream)
        if cut > 0:
            self._all_reduce_avg(self.flat.grad[:cut], late=True)
        for a in self.aux:
            if a["p"].requires_grad:
                self._all_reduce_avg(a["g"], late=True)
        self._timed_wait(lambda main: main.wait_event(self._ev_early))

    def _exchange_tail(self):
        self._settle(self._works_late)
        self._timed_wait(lambda main: main.wait_stream(self.comm_stream))

    def _timed_wait(self, wait):
        main = torch.cuda.current_stream(self.dev)
        if not self._time_comm:
            wait(main)
            return
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(main)
        wait(main)
        e1.record(main)
        self._comm_ev.append((e0, e1))

    def reset_comm_timing(self, enable=True):
        """Start (or stop) recording event pairs around the compute stream's waits for the gradient all-reduces."""
        self._comm_ev, self._time_comm = [], bool(enable)

    def exposed_comm_ms(self):
        """Total time the compute stream spent blocked on gradient all-reduces since reset_comm_timing() (the two wait points of
        a step: before Adam on the tail of the buffer, before Adam on its head).  Call after a device synchronisation."""
        tot = 0.0
        for e0, e1 in self._comm_ev:
            tot += e0.elapsed_time(e1)
        return tot

    # ------------------------------------------------------------------------------------------------------------
    # one training step
    # ------------------------------------------------------------------------------------------------------------
    def forward_backward(self, input_ids, attention_mask, training=True, compute_grads=True, dec_ids=None, dec_mask=None,
                         want_logits=False, quantizer_training=None, stop_after_quantizer=False, defer_backward=False, target_ids=None,
                         latents=None, stop_after_encoder=False, skip_quantizer=False, want_latents=False):
        """Forward (+ backward when compute_grads).  Returns dict(loss_recon, loss_vq, perplexity, acc, acc_per_sentence,
        recon_ids, indices [, logits] [, loss_tokens]).  loss_ignore_pad: loss_recon, its gradient, acc and
        acc_per_sentence run over the positions whose target is not the pad id, loss_tokens is their number (a device scalar) and
        recon_ids carries the pad id at the others.  dec_ids / dec_mask: the decoder's own input (Bagon.forward takes one, and the Bagon step
        tokenises and perturbs the two sides separately, models/bagon/Trainer.py:78-96; default = the encoder's).  target_ids:
        what the loss and the accuracy score the logits against (default = the decoder's input, as models/bagon/Trainer.py:103-110
        and models/shelgon3/Trainer.py:94-101 do).
        defer_backward (with compute_grads=False): the forward's activations stay alive and out["_resume"] can be handed to
        backward_from() once the gradient of the returned logits is known (kvq.engine.engine_autograd_forward).
        The latent calls (encode / decode below; forward-only, None / False everywhere else) enter and leave the same schedule:
        latents [B, Se, H] replaces the encoder's output (input_ids / attention_mask are not read and may be None),
        stop_after_encoder returns before the quantiser, skip_quantizer hands the encoder output (or `latents`) to the decoder as it
        is, want_latents adds z / z_q to what stop_after_quantizer returns."""
        if compute_grads:
            self._wema_refuse("forward_backward(compute_grads=True)")
        self._stop_after_quantizer = bool(stop_after_quantizer) and not compute_grads
        if (latents is not None or stop_after_encoder or skip_quantizer or want_latents) and (compute_grads or defer_backward):
            raise KvqError("TrainEngine: latents / stop_after_encoder / skip_quantizer / want_latents are forward-only arguments")
        enc_shape = tuple(latents.shape[:2]) if latents is not None else tuple(input_ids.shape)
        S = max(enc_shape[1], dec_ids.shape[1] if dec_ids is not None else 0)
        if S > (128 if self.dtype == torch.bfloat16 else 32):
            raise KvqError(f"TrainEngine: sequence length {S} above the attention kernels' limit (32 tokens in f32, 128 in bf16 "
                           f"through the blocked kernels; use the autograd path)")
        if dec_ids is not None and (dec_mask is None or dec_ids.shape[0] != enc_shape[0] or dec_mask.shape != dec_ids.shape):
            raise KvqError("TrainEngine: dec_ids needs a dec_mask of its shape and the encoder's batch size")
        if target_ids is not None and target_ids.shape != (dec_ids if dec_ids is not None else input_ids).shape:
            raise KvqError("TrainEngine: target_ids must have the shape of the decoder's input")
        if defer_backward and (compute_grads or self._cap is not None or self._dp):
            raise KvqError("TrainEngine: defer_backward is a single-process, eager, forward-first call")
        self._site_ctr = 0
        self._red_items, self._red_keep = [], []
        self._wg_reset()
        pre = getattr(self, "_prepared", None) or {}            # this batch's (sorted ids, order) per side: _normalise_prepared()
        self._sorted = {"enc.emb.": pre.get("enc"), "dec.emb.": pre.get("dec") if dec_ids is not None else "enc.emb."}
        # dropout seeds of this engine's launches = _step_seed + device step count (grad_accum > 1: + device micro-step count)
        nnops.set_seed_offset(self._seed_state)
        if compute_grads:
            self._grads_are_mean = False       # the flat gradient is this call's again (train_step says when the accumulator is the mean)
        self._in_fb = True
        try:
            self._q_training = training if quantizer_training is None else bool(quantizer_training)
            with torch.no_grad():            # the schedule IS the backward pass: no autograd graph over the few torch ops in it
                if self.fp8:
                    self._x8.clear()
                self._fp8_bwd_begin(compute_grads)
                out = self._forward_backward(input_ids, attention_mask, training, compute_grads, dec_ids, dec_mask, want_logits,
                                             defer=bool(defer_backward), target_ids=target_ids, latents=latents,
                                             stop_after_encoder=bool(stop_after_encoder), skip_quantizer=bool(skip_quantizer),
                                             want_latents=bool(want_latents))
                if defer_backward:
                    out["_resume"] = dict(gen=out.pop("_gen"), sorted_ids=self._sorted, step=self._step_host,
                                          versions=self._versions())
                self._fp8_bwd_end()
                if self.fp8 and compute_grads:
                    # the next TRAINING step's activation scales from this step's amax (4x headroom).  A forward-only call
                    # (evaluation, Shelgon.forward) uses the scales as they are and leaves them alone: an eval batch must not
                    # move the scales of the training step that follows it
                    check(lib().kvq_fp8_update_scales(self._a8_state.data_ptr(), self._a8_sites, 4.0, stream_ptr()), "kvq_fp8_update_scales")
                elif self.fp8:
                    # (the producers note amax by atomic maxima: what an evaluation batch left in the partial slots must go)
                    check(lib().kvq_fp8_update_scales(self._a8_state.data_ptr(), self._a8_sites, 0.0, stream_ptr()), "kvq_fp8_update_scales")
                return out
        finally:
            self._bwd8_mode = None
            self._in_fb = False
            nnops.set_seed_offset(None)

    def forward_logits(self, enc_ids, enc_mask, dec_ids=None, dec_mask=None, training=False, quantizer_training=None):
        """Forward only, on the engine's kernels, with the [B, S, V] logits in the result: what Bagon.forward / Shelgon.forward
        return (models/bagon/Bagon.py:40-55, models/shelgon3/Shelgon.py:50-73)."""
        self.refresh_if_params_changed()
        self._distrust_codebook_pack()         # an evaluation forward never trusts a cached pack (a 3-us kernel; see _codebook_stamp)
        return self.forward_backward(enc_ids, enc_mask, training=training, compute_grads=False, dec_ids=dec_ids, dec_mask=dec_mask,
                                     want_logits=True, quantizer_training=quantizer_training)

    def code_indices(self, enc_ids, enc_mask, quantizer_training=False):
        """Encoder + quantiser only: dict(indices, perplexity, loss_vq_raw).  What a consumer of the codes needs -- the reference's
        analysis (analyses/unsupervised_vq_disentanglement/unsupervised_vq_disentanglement.py:164) runs the whole model.forward
        and drops everything but min_encoding_indices; the decoder and the LM head are 60 % of a forward."""
        if not self.has_vq:
            raise KvqError("TrainEngine.code_indices: the model has no quantiser")
        self.refresh_if_params_changed()
        self._distrust_codebook_pack()
        return self.forward_backward(enc_ids, enc_mask, training=False, compute_grads=False, quantizer_training=quantizer_training,
                                     stop_after_quantizer=True)

    def _forward_backward(self, input_ids, attention_mask, training, compute_grads, dec_ids=None, dec_mask=None, want_logits=False,
                          defer=False, target_ids=None, latents=None, stop_after_encoder=False, skip_quantizer=False,
                          want_latents=False):
        gen = self._fb_gen(input_ids, attention_mask, training, compute_grads, dec_ids, dec_mask, want_logits, defer, target_ids,
                           latents, stop_after_encoder, skip_quantizer, want_latents)
        try:
            out = next(gen)                 # only a deferred call yields: forward done, the generator holds the activations
        except StopIteration as done:
            return done.value
        out["_gen"] = gen
        return out

    def backward_from(self, resume, g_logits, g_loss_vq=None):
        """The backward half of a forward_backward(..., defer_backward=True) call, seeded with d L / d logits ([B, S, V], the
        logits' dtype) and d L / d loss_vq_raw (scalar tensor or None = 0) instead of this engine's own loss: gradients land in
        the flat buffer exactly as in a training step (grads_by_parameter() hands them out)."""
        if resume.get("done"):
            raise KvqError("TrainEngine.backward_from: this forward's activations were already consumed")
        if resume["step"] != self._step_host or resume["versions"] != self._versions():
            raise KvqError("TrainEngine.backward_from: parameters changed since the forward (an optimiser step or an in-place write)")
        resume["done"] = True
        self._red_items, self._red_keep = [], []
        self._wg_reset()
        self._sorted = resume["sorted_ids"]
        self._g_vq_ext = (g_loss_vq.detach().to(torch.float32).reshape(()) if g_loss_vq is not None
                          else torch.zeros((), dtype=torch.float32, device=self.dev)) if self.has_vq else None
        nnops.set_seed_offset(self._seed_state)     # the step count has not moved: backward regenerates the forward's dropout masks
        self._grads_are_mean = False
        try:
            with torch.no_grad():
                try:
                    resume["gen"].send(g_logits.detach())
                except StopIteration:
                    pass
                else:
                    raise KvqError("TrainEngine.backward_from: the schedule did not finish")
        finally:
            nnops.set_seed_offset(None)
            self._g_vq_ext = None

    def grads_by_parameter(self):
        """{nn.Parameter: float32 gradient} of the last backward, for every trainable parameter of the model (what autograd would
        have put into .grad): views of the flat bf16 / f32 gradient buffer converted to the parameter's dtype.  grad_accum > 1:
        after a train_step that ran the optimiser, the mean over the cycle's micro-batches (what Adam read); after any other
        call, that micro-batch's own gradient."""
        out = {}
        mean = self._grads_are_mean
        for name, p in self.param_of.items():
            if p.requires_grad:
                o, n, shape = self.flat.seg[name]
                g = self.flat.acc[o:o + n].view(shape) if mean else self.flat.g(name)
                out[p] = torch.empty_like(p).copy_(g.reshape(p.shape))           # a copy: the flat buffer is rewritten by the next backward
        for a in self.aux:
            if a["p"].requires_grad:
                out[a["p"]] = torch.empty_like(a["p"]).copy_(a["acc" if mean else "g"].reshape(a["p"].shape))
        return out

    def _fb_gen(self, input_ids, attention_mask, training, compute_grads, dec_ids, dec_mask, want_logits, defer, target_ids=None,
                latents=None, stop_after_encoder=False, skip_quantizer=False, want_latents=False):
        m = self.model
        fl, H = self.flat, self.H
        B, S = latents.shape[:2] if latents is not None else input_ids.shape
        N = B * S
        mask = attention_mask.contiguous() if attention_mask is not None else None
        ecfg, dcfg = self.ecfg, self.dcfg
        d_ids = input_ids if dec_ids is None else dec_ids
        d_mask = mask if dec_mask is None else dec_mask.contiguous()
        Sd = d_ids.shape[1]
        Nd = B * Sd
        if d_ids.shape[0] != B:
            raise KvqError("TrainEngine: encoder and decoder batches differ")

        # ---------------- forward ----------------
        enc_saved = []
        if latents is not None:             # decode(): the caller's latent stands where the encoder's output would
            x, emb_saved = latents.view(N, H), None
        else:
            x, emb_saved = self._emb_fwd("enc.emb.", ecfg, input_ids, training)
            for i in range(self.n_enc_layers):
                x, sa = self._attn_block_fwd(f"enc.{i}.sa.", x, None, mask, False, ecfg, training, B, S, S, next_key=f"enc.{i}.f1.w")
                x, ff = self._ffn_fwd(f"enc.{i}.", x, ecfg, training, next_key=f"enc.{i + 1}.sa.q.w" if i + 1 < self.n_enc_layers else None)
                enc_saved.append((sa, ff))
        z = x
        if stop_after_encoder:              # encode() without a quantiser, or with quantize=False
            return dict(z=z.view(B, S, H))
        gum_saved = None
        if skip_quantizer:                  # decode(quantize=False) of a model with a quantiser: the latent goes to the decoder as it is
            idx, loss_vq, perplexity, enc_out, indices = None, None, None, z, None
        elif self.vq_kind in ("VectorQuantizer", "MultiVectorQuantizer"):
            cap = self._cap
            if cap is not None:                     # graph capture: the quantiser stays an eager launch between two graphs
                z_q, idx, vq_out = cap.z_q, cap.idx, cap.vq_out
            else:
                z_q = torch.empty_like(z)
                idx = torch.empty(N * self.G, dtype=torch.int64, device=self.dev)
                vq_out = torch.empty(2, dtype=torch.float32, device=self.dev)
            revive = compute_grads and self.revive_after is not None        # training steps only
            self._eager(lambda: self._vq_forward(z, z_q, idx, vq_out, revive))
            loss_vq, perplexity = vq_out[0], vq_out[1]
            enc_out = z_q
            indices = idx.view(self.G, N).t().reshape(B, S, self.G)          # [B, S, 1] for the reference's single codebook
        elif self.vq_kind == "GumbelQuantizer":
            enc_out, loss_vq, perplexity, ind, gum_saved = self._gumbel_forward(z, self._q_training)
            idx, indices = ind, ind.view(B, S)                               # GumbelQuantizer.py:76 returns [B, S]
        else:
            idx, loss_vq, perplexity, enc_out, indices = None, None, None, z, None
        if getattr(self, "_stop_after_quantizer", False):
            if want_latents:                # encode()
                return dict(z=z.view(B, S, H), z_q=enc_out.view(B, S, H), indices=indices, perplexity=perplexity, loss_vq_raw=loss_vq)
            return dict(indices=indices, perplexity=perplexity, loss_vq_raw=loss_vq)

        y, demb_saved = self._emb_fwd("dec.emb.", dcfg, d_ids, training, word_rows=None)
        dec_saved = []
        kv_all = None
        if self._cakv_batched:             # keys | values of every decoder layer's cross-attention in one [N, L*2H] GEMM
            kv_all = self._linear(enc_out, None, None, Wb=(fl.fused(self._cakv_w, fl.shadow), fl.fused(self._cakv_b, fl.shadow)),
                                  key=self._cakv_w[0])
        for i in range(self.n_dec_layers):
            y, sa = self._attn_block_fwd(f"dec.{i}.sa.", y, None, d_mask, True, dcfg, training, B, Sd, Sd, next_key=f"dec.{i}.ca.q.w")
            y, ca = self._attn_block_fwd(f"dec.{i}.ca.", y, enc_out, None, False, dcfg, training, B, Sd, S,
                                         kv_pre=kv_all[:, 2 * H * i: 2 * H * (i + 1)] if kv_all is not None else None,
                                         next_key=f"dec.{i}.f1.w")
            y, ff = self._ffn_fwd(f"dec.{i}.", y, dcfg, training, next_key=f"dec.{i + 1}.sa.q.w" if i + 1 < self.n_dec_layers else "head.t.w")
            dec_saved.append((sa, ca, ff))
        t, ta = self._linear_gelu(y, "head.t.w", "head.t.b")
        if self.fp8 and "dec.emb.word" in self._w8_index and ta.dtype == torch.bfloat16 and os.environ.get("KVQ_FP8_HEAD_EMIT", "1") != "0":
            # the LM head runs on fp8 in every fp8 scope: the LayerNorm in front of it writes the fp8 copy of its output itself
            hN, hpre, hmean, hrstd, hN8 = nnops.ln_fwd_fp8(ta, None, fl.w32("head.ln.w"), fl.w32("head.ln.b"), dcfg.layer_norm_eps, 0.0, 0, 0,
                                                           self._a8_state_of("dec.emb.word"))
            self._x8[(hN.data_ptr(), "dec.emb.word")] = hN8
        else:
            hN, hpre, hmean, hrstd = nnops.ln_fwd(ta, None, fl.w32("head.ln.w"), fl.w32("head.ln.b"), dcfg.layer_norm_eps)
        Wv = fl.w("dec.emb.word", rows=self.Vp)                              # [Vp,H], rows >= V are zero
        bv = fl.shadow[fl.seg["head.bias"][0]: fl.seg["head.bias"][0] + self.Vp]
        tgt = (d_ids if target_ids is None else target_ids).reshape(-1)
        # LM head; with the own kernel its epilogue also leaves the loss' forward statistics per (row, 256-column tile): the
        # [N, Vp] logits are then read by the loss only once more, in backward (opt-in, KVQ_OWN_LMCE=1; default: library GEMM + kvq_ce_forward)
        lm_stats = None
        if self._own_lmce and self._own_fwd and not self.fp8 and self.dtype == torch.bfloat16 and hN.shape[0] >= 2048 \
                and hN.is_contiguous() and self.Vp % 8 == 0:
            logits, lm_stats = nnops.gemm_ce(hN, Wv, bv, self.V)
        else:
            logits = self._linear(hN, None, None, Wb=(Wv, bv), key="dec.emb.word")  # [N,Vp]
        row_loss = torch.empty(Nd, dtype=torch.float32, device=self.dev)
        row_lse = torch.empty(Nd, dtype=torch.float32, device=self.dev)
        pred = torch.empty(Nd, dtype=torch.int64, device=self.dev)
        ign = self._pad_idx if self.loss_ignore_pad else None      # loss_ignore_pad: rows whose target is the pad id are left out
        ce_cnt = None
        if self._cap is not None and compute_grads:
            ce_out = self._cap.scal[0:2]
            if ign is not None:
                ce_cnt = self._cap.scal[4:5]
        elif ign is not None:
            ce_out = torch.empty(3, dtype=torch.float32, device=self.dev)
            ce_cnt = ce_out[2:3]
        else:
            ce_out = torch.empty(2, dtype=torch.float32, device=self.dev)
        if lm_stats is not None:
            nnops.ce_forward_stats(logits, tgt, lm_stats, row_loss, row_lse, pred, ce_out[0:], ce_out[1:], ignore_index=ign, count=ce_cnt)
        else:
            nnops.ce_forward(logits, tgt, self.V, self.Vp, row_loss, row_lse, pred, ce_out[0:], ce_out[1:], ignore_index=ign, count=ce_cnt)
        acc_sent = None
        if self.sentence_acc or latents is not None:     # seq_acc's second result (common/metrics.py:32-36), read by the Bagon trainer's decode step
            acc_sent = torch.empty(B, dtype=torch.float32, device=self.dev)
            nnops.seq_acc(pred, tgt, B, Sd, acc_sent, ignore_index=ign)
        out = dict(loss_recon=ce_out[0] if self.w_recon == 1.0 else ce_out[0] * self.w_recon,
                   loss_vq=(loss_vq if self.w_vq == 1.0 else loss_vq * self.w_vq) if loss_vq is not None else None,
                   perplexity=perplexity, acc=ce_out[1], acc_per_sentence=acc_sent, recon_ids=pred.view(B, Sd), indices=indices)
        if ign is not None:
            out["loss_tokens"] = ce_cnt[0]                        # the number of counted tokens, a device scalar (f32, exact)
        if want_logits:
            out["logits"] = logits[:, :self.V].reshape(B, Sd, self.V)
            out["loss_vq_raw"] = loss_vq                          # without the trainer's loss weight
        g_ext = None
        if not compute_grads:
            if not defer:
                return out
            g_ext = yield out               # suspended here until backward_from() sends d L / d logits

        # ---------------- backward ----------------
        tr = fl.trainable
        g_scale = self._g_recon
        if g_ext is not None:
            # the caller's loss: its gradient replaces this engine's (the [N, V] part of a fresh [N, Vp] buffer -- the logits handed
            # out stay as they are)
            g_logits = torch.zeros_like(logits)
            g_logits[:, :self.V].copy_(g_ext.reshape(Nd, self.V))
            if tr["head.bias"]:
                self._defer_colsum(g_logits, fl.g("head.bias", rows=self.Vp))
        elif tr["head.bias"] and self.Vp % 8 == 0:
            # in place: logits := d loss / d logits; the LM-head bias gradient leaves the same pass as partial column sums
            pb = torch.empty((nnops.ce_bwd_partial_rows(Nd), self.Vp), dtype=torch.float32, device=self.dev)
            # (with ign the count is read from the slot the forward's finalize wrote, on the device)
            nnops.ce_backward_bias(logits, tgt, row_lse, g_scale, self.V, self.Vp, logits, pb, ignore_index=ign, count=ce_cnt)
            self._defer(pb, fl.g("head.bias", rows=self.Vp), pb.shape[0], self.Vp, self.Vp)
            g_logits = logits
        else:
            nnops.ce_backward(logits, tgt, row_lse, g_scale, self.V, self.Vp, logits, ignore_index=ign, count=ce_cnt)      # in place
            g_logits = logits
            if tr["head.bias"]:
                self._defer_colsum(g_logits, fl.g("head.bias", rows=self.Vp))
        if tr["dec.emb.word"]:
            self._wgrad(g_logits, hN, fl.g("dec.emb.word", rows=self.Vp))            # [Vp,H] = g_logits^T hN
        g_hN = self._dgrad(g_logits, Wv, key="dec.emb.word")      # (contracts over the padded vocabulary, 238.5 x 128: bf16)
        del logits, g_logits
        g_ta, _ = self._ln_bwd(g_hN, hpre, hmean, hrstd, fl.w32("head.ln.w"), 0.0, 0, 0,
                               g_gamma=fl.g("head.ln.w") if tr["head.ln.w"] else None,
                               g_beta=fl.g("head.ln.b") if tr["head.ln.b"] else None, need_g_resid=False)
        if tr["head.t.b"] and t.is_contiguous() and t.shape[1] % 8 == 0:
            g_t, pb = nnops.gelu_bwd_bias(t, g_ta, out=g_ta)
            self._defer(pb, fl.g("head.t.b"), pb.shape[0], pb.shape[1], pb.shape[1])
            g_y = self._linear_bwd(g_t, y, ["head.t.w"], ["head.t.b"], bias_done=True, fill_unit=256)
        else:
            g_t = nnops.gelu_bwd(t, g_ta, out=g_ta)
            g_y = self._linear_bwd(g_t, y, ["head.t.w"], ["head.t.b"], fill_unit=256)
        self._grads_done_down_to("head.t.w")
        g_kv_all = pb_kv_all = None
        if self._cakv_batched:
            g_kv_all = torch.empty_like(kv_all)
            if tr[self._cakv_b[0]]:
                pb_kv_all = torch.empty((B, kv_all.shape[1]), dtype=torch.float32, device=self.dev)
            g_enc = None
        else:
            g_enc = torch.zeros_like(enc_out)
        for i in reversed(range(self.n_dec_layers)):
            sa, ca, ff = dec_saved[i]
            g_y = self._ffn_bwd(f"dec.{i}.", g_y, ff)
            sl = slice(2 * H * i, 2 * H * (i + 1))
            g_y = self._attn_block_bwd(f"dec.{i}.ca.", g_y, ca, g_kv_src=g_enc,
                                       g_kv_out=g_kv_all[:, sl] if g_kv_all is not None else None,
                                       pb_kv_out=pb_kv_all[:, sl] if pb_kv_all is not None else None)
            g_y = self._attn_block_bwd(f"dec.{i}.sa.", g_y, sa)
            self._grads_done_down_to(f"dec.{i}.sa.q.w")
            dec_saved[i] = None
        if self._cakv_batched:             # all layers' key/value projections at once: weight, bias and input gradients
            if tr[self._cakv_w[0]]:
                self._wgrad_fill(g_kv_all, enc_out, fl.fused(self._cakv_w, fl.grad), 2 * H)      # per-layer slices
            if pb_kv_all is not None:
                self._defer(pb_kv_all, fl.fused(self._cakv_b, fl.grad), B, pb_kv_all.shape[1], pb_kv_all.shape[1])
            g_enc = self._dgrad(g_kv_all, fl.fused(self._cakv_w, fl.shadow), key=self._cakv_w[0])
            del g_kv_all, kv_all
            self._grads_done_down_to(self._cakv_w[0])
        self._emb_bwd("dec.emb.", g_y, demb_saved, tied_accumulate=True)
        self._grads_done_down_to("dec.emb.word")
        if self.vq_kind in ("VectorQuantizer", "MultiVectorQuantizer"):
            g_x = self._vq_backward(z, idx, g_enc)
        elif self.vq_kind == "GumbelQuantizer":
            g_x = self._gumbel_backward(g_enc, gum_saved)
        else:
            g_x = g_enc
        any_enc = any(v for k, v in tr.items() if k.startswith("enc."))
        if any_enc:
            for i in reversed(range(self.n_enc_layers)):
                sa, ff = enc_saved[i]
                g_x = self._ffn_bwd(f"enc.{i}.", g_x, ff)
                g_x = self._attn_block_bwd(f"enc.{i}.sa.", g_x, sa)
                self._grads_done_down_to(f"enc.{i}.sa.q.w", partial=(i == 0))
                enc_saved[i] = None
            self._emb_bwd("enc.emb.", g_x, emb_saved)
        self._flush_reductions()
        return out

    def _buf(self, name, shape, dtype):
        """Persistent scratch of the eager (between-graphs) launches: same storage every step."""
        key = (name, tuple(shape), dtype)
        t = self._bufs.get(key)
        if t is None:
            t = self._bufs[key] = torch.empty(shape, dtype=dtype, device=self.dev)
        return t

    def _repack_codebook(self):
        if self._epack is not None:
            check(lib().kvq_vq_pack_codebook(self.E.data_ptr(), self.K, self.Dg, self.G, self._epack.data_ptr(), stream_ptr()),
                  "kvq_vq_pack_codebook")
            self._E_version = self._codebook_stamp()

    def _distrust_codebook_pack(self):
        """The next quantiser call repacks the codebook.  (getattr: some callers run before __init__ has made the pack, and a model
        without an arg-min quantiser has none.  _E_version is read only where there is a pack.)"""
        if getattr(self, "_epack", None) is not None:
            self._E_version = None

    def _codebook_stamp(self):
        """What tells a codebook write from outside: the tensor version (in-place torch ops, optimiser steps) and the module's
        epoch counter (its EMA kernel writes through a raw pointer).  A `.data` write that bumps neither needs
        sync_from_model(); forward_logits() repacks unconditionally."""
        return (self.E._version, getattr(self.model.vector_quantizer, "codebook_epoch", 0))

    def _vq_fwd_call(self, z, N, D, G, z_q, idx, loss, perp, ws):
        if self._epack is None:
            check(lib().kvq_vq_forward(z.data_ptr(), self.E.data_ptr(), N, self.K, D, G, self.io, self.beta_vq, z_q.data_ptr(),
                                       idx.data_ptr(), loss.data_ptr(), perp.data_ptr(), None, ws.data_ptr(), ws.numel(), stream_ptr()),
                  "kvq_vq_forward")
            return
        if self._codebook_stamp() != self._E_version:   # first call, or the codebook was written from outside the engine
            self._repack_codebook()
        check(lib().kvq_vq_forward_packed(z.data_ptr(), self.E.data_ptr(), self._epack.data_ptr(), N, self.K, D, G, self.io,
                                          self.beta_vq, z_q.data_ptr(), idx.data_ptr(), loss.data_ptr(), perp.data_ptr(), None,
                                          ws.data_ptr(), ws.numel(), stream_ptr()), "kvq_vq_forward_packed")

    def _vq_forward(self, z, z_q, idx, vq_out, revive=False):
        """kvq_vq_forward on the encoder output: one codebook (the reference's VectorQuantizer), or G codebooks on G column
        slices as one grouped launch (MultiVectorQuantizer: loss / perplexity = mean over the factors)."""
        N, H = z.shape
        G, K, Dg = self.G, self.K, self.Dg
        ws = _workspace(self.dev, lib().kvq_vq_workspace_bytes(N, K, Dg, G))
        if G == 1:
            self._vq_fwd_call(z, N, H, 1, z_q, idx, vq_out[0:], vq_out[1:], ws)
            zsrc = z
        else:
            vq = self.model.vector_quantizer
            zg = self._buf("zg", (G, N, Dg), z.dtype)
            zg.copy_(vq.split(z))
            zqg = self._buf("zqg", (G, N, Dg), z.dtype)
            lp = self._buf("lp", (2, G), torch.float32)
            self._vq_fwd_call(zg, N, Dg, G, zqg, idx, lp[0], lp[1], ws)
            z_q.copy_(vq.merge(zqg))
            vq_out[0:1].copy_(lp[0].sum(0, keepdim=True) * vq.loss_weight)          # (1 + beta) * MSE over all N * e_dim elements
            vq_out[1:2].copy_(lp[1].mean(0, keepdim=True))
            zsrc = zg
        if self.vq_ema:                      # the EMA step runs after backward: keep what it needs in storage of its own
            self._buf("ema_z", zsrc.shape, zsrc.dtype).copy_(zsrc)
            self._buf("ema_idx", idx.shape, idx.dtype).copy_(idx)
            self._ema_shapes = (tuple(zsrc.shape), zsrc.dtype, tuple(idx.shape))
        if revive:
            self._revive_select(zsrc, idx)

    def _revive_select(self, zsrc, idx):
        """Codebook revival, first half, in the quantiser's interlude where z and idx are live: usage flags, idle counters and
        the donor rows of the codes that are now dead (kvq.functional.vq_revive_select; data parallel: its two small all-reduces
        sit in the hand-over between the step's graphs).  The kernel's seed is _step_seed + the device step count BEFORE this
        step's kvq_step_state_advance -- the seed of this step's dropout masks.  A replayed interlude runs outside
        forward_backward(): it sets the seed offset itself."""
        self._rv_pending = True
        if self._cap is not None:          # capture runs an interlude once on the unwritten buffers of graphs that have not run:
            return                         # that is no training step -- idle does not advance; the replays (no _cap) do the work
        if self.revive_keep_donors:
            self._buf("revive_z", (self.G, zsrc.shape[-2], self.Dg), zsrc.dtype).copy_(zsrc.view(self.G, -1, self.Dg))
            self._rv_donor_shape = ((self.G, zsrc.shape[-2], self.Dg), zsrc.dtype)
        nnops.set_seed_offset(self._seed_state)
        try:
            vq_revive_select(zsrc, idx, self._rv_idle, self.E.data, self.revive_after, self._step_seed, used=self._rv_used,
                             rows=self._rv_rows, group=self.group)
        finally:
            if not self._in_fb:
                nnops.set_seed_offset(None)

    def _revive_apply(self):
        """Second half, behind the codebook's own update (Adam on the aux parameters, or the EMA step) and before the codebook is
        repacked: the dead codes take their rows, their moments restart.  Not gated by the gradient guard's skip."""
        if not self._rv_pending:
            return
        self._rv_pending = False
        vq = self.model.vector_quantizer
        a = next((x for x in self.aux if x["p"] is self.E), None) if self.E.requires_grad else None
        vq_revive_apply(self._rv_rows, self._rv_idle, self.E.data, self.revive_after, self._rv_counter,
                        m=a["m"] if a else None, v=a["v"] if a else None, vmax=a["vmax"] if a else None,
                        ema_n=vq.ema_n if self.vq_ema else None, ema_m=vq.ema_m if self.vq_ema else None)

    @property
    def code_idle(self):
        """[G, K] int32 view of the idle counters (revive_after only; None otherwise): training steps since code k of codebook g
        last won a token."""
        return self._rv_idle.view(self.G, self.K) if self.revive_after is not None else None

    @property
    def revived_codes(self):
        """Codes revived so far (revive_after only; synchronises)."""
        return read_revive_counter(self._rv_counter)["total"] if self.revive_after is not None else 0

    @property
    def revive_donors(self):
        """[G, N, D] copy of the encoder outputs the last select kernel drew its donors from (revive_keep_donors = True only)."""
        shape, dt = self._rv_donor_shape
        return self._buf("revive_z", shape, dt)

    def _vq_backward(self, z, idx, g_enc):
        N, H = z.shape
        G, K, Dg = self.G, self.K, self.Dg
        ws = _workspace(self.dev, lib().kvq_vq_workspace_bytes(N, K, Dg, G))
        gE = self.gE.data_ptr() if self.E.requires_grad else None
        if G == 1:
            g_z = torch.empty_like(z)
            gl = self._g_vq if self._g_vq_ext is None else self._g_vq_ext
            check(lib().kvq_vq_backward(z.data_ptr(), self.E.data_ptr(), idx.data_ptr(), g_enc.data_ptr(), gl.data_ptr(), N, K, H, 1,
                                        self.io, self.beta_vq, g_z.data_ptr(), gE, ws.data_ptr(), ws.numel(), stream_ptr()),
                  "kvq_vq_backward")
            return g_z
        vq = self.model.vector_quantizer
        zg, gq = vq.split(z), vq.split(g_enc)
        if self._g_vq_ext is None:
            gl = torch.full((G,), self.w_vq * vq.loss_weight, dtype=torch.float32, device=self.dev)
        else:
            gl = (self._g_vq_ext * vq.loss_weight).expand(G).contiguous()
        gzg = torch.empty_like(zg)
        check(lib().kvq_vq_backward(zg.data_ptr(), self.E.data_ptr(), idx.data_ptr(), gq.data_ptr(), gl.data_ptr(), N, K, Dg, G,
                                    self.io, self.beta_vq, gzg.data_ptr(), gE, ws.data_ptr(), ws.numel(), stream_ptr()),
              "kvq_vq_backward")
        return vq.merge(gzg)

    def _ema_step(self):
        if self._cap is not None:          # capture runs an interlude once on the unwritten buffers of graphs that have not run:
            return                         # that is no training step -- the statistics do not move; the replays (no _cap) do the work
        zs, zdt, ishape = self._ema_shapes
        z, idx = self._buf("ema_z", zs, zdt), self._buf("ema_idx", ishape, torch.int64)
        self.model.vector_quantizer.ema_update(z, idx.view(self.G, -1) if self.G > 1 else idx)
        self._repack_codebook()

    # ---- GumbelQuantizer (models/shelgon3/GumbelQuantizer.py:43-83): 1x1 conv = GEMM, row kernel, codebook GEMM ----------------
    def _mm(self, a, b, layout, bias=None):
        """op(a) . op(b) (+ bias) for the six products of the Gumbel mode (n_embed = 512 codes meets the MFMA kernel's requirements,
        the reference analysis' 9 codes go to the any-shape kernel).  layout as nnops.gemm: "nt" | "nn" | "tn"."""
        if self._own_fwd and self.dtype == torch.bfloat16:
            self._gumbel_own += 1
        return self._gemm(a, b, layout, bias=bias)

    def _gumbel_forward(self, z, training):
        gq = self.model.vector_quantizer
        N, H = z.shape
        K, dt = gq.n_embed, self.dtype
        Wp = gq.proj.weight.squeeze(-1).to(dt)                                        # [K, H]
        logits = self._mm(z, Wp, "nt", bias=gq.proj.bias.to(dt))
        hard = bool(gq.straight_through) if training else True                       # :54
        y = torch.empty_like(logits)
        y_soft = torch.empty((N, K), dtype=torch.float32, device=self.dev)
        ind = torch.empty(N, dtype=torch.int64, device=self.dev)
        kl_row = torch.empty(N, dtype=torch.float32, device=self.dev)
        noise = getattr(self, "gumbel_noise", None)           # tests: explicit Gumbel(0,1) samples [N, K] f32 instead of the Philox stream
        check(lib().kvq_gumbel_forward(logits.data_ptr(), noise.data_ptr() if noise is not None else None, N, K,
                                       float(gq.temperature), int(hard), int(self._step_seed), self._site(),
                                       self.io, y.data_ptr(), y_soft.data_ptr(), ind.data_ptr(), kl_row.data_ptr(), stream_ptr()),
              "kvq_gumbel_forward")
        diff = kl_row.mean() * float(gq.kld_scale)                                    # :73
        emb = gq.embed.weight.to(dt)
        z_q = self._mm(y, emb, "nn")                                                  # :66 einsum, already [N, D]
        used = torch.zeros(K, dtype=torch.float32, device=self.dev).scatter_add_(0, ind, self._ones.expand(N))
        perplexity = (used > 0).sum().float()                                         # codes in use (Shelgon.py:63)
        return z_q, diff, perplexity, ind, (z, logits, y, y_soft, Wp, emb)

    def _gumbel_backward(self, g_zq, saved):
        gq = self.model.vector_quantizer
        z, logits, y, y_soft, Wp, emb = saved
        N, K = logits.shape
        g_y = self._mm(g_zq, emb, "nt")
        self.g_emb.copy_(self._mm(y, g_zq, "tn"))
        gd = self._ones.reshape(1) * self.w_vq if self._g_vq_ext is None else self._g_vq_ext.reshape(1)
        g_logits = torch.empty_like(logits)
        check(lib().kvq_gumbel_backward(logits.data_ptr(), y_soft.data_ptr(), g_y.data_ptr(), gd.data_ptr(), N, K, float(gq.temperature),
                                        float(gq.kld_scale), self.io, g_logits.data_ptr(), stream_ptr()), "kvq_gumbel_backward")
        self.g_pw.copy_(self._mm(g_logits, z, "tn").unsqueeze(-1))
        torch.sum(g_logits.float(), dim=0, out=self.g_pb)     # (out=: a same-dtype copy_ would be a memcpy NODE of a captured step)
        return self._mm(g_logits, Wp, "nn")

    @staticmethod
    def check_max_grad_norm(v, env=False):
        """None (off), or the float > 0 / float("inf") a TrainEngine(max_grad_norm=...) accepts; anything else raises KvqError.
        env: None means KVQ_MAX_GRAD_NORM from the environment (unset or empty: off)."""
        if v is None and env and os.environ.get("KVQ_MAX_GRAD_NORM", "") != "":
            try:
                v = float(os.environ["KVQ_MAX_GRAD_NORM"])
            except ValueError:
                raise KvqError(f"TrainEngine: KVQ_MAX_GRAD_NORM (max_grad_norm) must be a float > 0 or inf, got "
                               f"{os.environ['KVQ_MAX_GRAD_NORM']!r}") from None
        if v is None:
            return None
        if isinstance(v, bool) or not isinstance(v, (int, float)) or not v > 0:
            raise KvqError(f"TrainEngine: max_grad_norm must be None, a float > 0 or float('inf'), got {v!r}")
        return float(v)

    @staticmethod
    def check_grad_accum(v, env=False):
        """The int >= 1 a TrainEngine(grad_accum=...) accepts (1: off); anything else raises KvqError.  env: None means
        KVQ_GRAD_ACCUM from the environment (unset or empty: 1).  What grad_accum > 1 may not be combined with is refused by the
        constructor, which knows the model."""
        if v is None and env and os.environ.get("KVQ_GRAD_ACCUM", "") != "":
            try:
                v = int(os.environ["KVQ_GRAD_ACCUM"])
            except ValueError:
                raise KvqError(f"TrainEngine: KVQ_GRAD_ACCUM (grad_accum) must be an integer >= 1, got "
                               f"{os.environ['KVQ_GRAD_ACCUM']!r}") from None
        if v is None:
            return 1
        if isinstance(v, bool) or not isinstance(v, int) or v < 1:
            raise KvqError(f"TrainEngine: grad_accum must be None or an integer >= 1, got {v!r}")
        return v

    @staticmethod
    def check_loss_ignore_pad(v, env=False):
        """The bool a TrainEngine(loss_ignore_pad=...) accepts (False: off); anything else raises KvqError.  env: None means
        KVQ_LOSS_IGNORE_PAD from the environment (unset, empty or 0: off; 1: on).  That the model has a pad id is checked by the
        constructor, which knows the model."""
        if v is None and env and os.environ.get("KVQ_LOSS_IGNORE_PAD", "") != "":
            s = os.environ["KVQ_LOSS_IGNORE_PAD"]
            if s not in ("0", "1"):
                raise KvqError(f"TrainEngine: KVQ_LOSS_IGNORE_PAD (loss_ignore_pad) must be 0 or 1, got {s!r}")
            v = s == "1"
        if v is None:
            return False
        if not isinstance(v, bool):
            raise KvqError(f"TrainEngine: loss_ignore_pad must be None, False or True, got {v!r}")
        return v

    @staticmethod
    def check_weight_ema(v, env=False):
        """None (off), or the float in (0, 1) a TrainEngine(weight_ema=...) accepts; anything else raises KvqError.
        env: None means KVQ_WEIGHT_EMA from the environment (unset or empty: off)."""
        if v is None and env and os.environ.get("KVQ_WEIGHT_EMA", "") != "":
            try:
                v = float(os.environ["KVQ_WEIGHT_EMA"])
            except ValueError:
                raise KvqError(f"TrainEngine: KVQ_WEIGHT_EMA (weight_ema) must be a float in (0, 1), got "
                               f"{os.environ['KVQ_WEIGHT_EMA']!r}") from None
        if v is None:
            return None
        if isinstance(v, bool) or not isinstance(v, (int, float)) or not 0 < v < 1:
            raise KvqError(f"TrainEngine: weight_ema must be None or a float in (0, 1), got {v!r}")
        return float(v)

    # ---- parameter groups, decoupled weight decay, learning-rate schedule -----------------------------------
    @staticmethod
    def _env_value(name, parse, what):
        s = os.environ.get(name, "")
        if s == "":
            return None
        try:
            return parse(s)
        except ValueError:
            raise KvqError(f"TrainEngine: {name} must be {what}, got {s!r}") from None

    @staticmethod
    def check_param_groups(v, env=False):
        """None (off), or the normalised list of {"match": [patterns], "lr_scale": float, "weight_decay": float | None (the engine's)}
        a TrainEngine(param_groups=...) accepts; anything else raises KvqError naming the offender.  env: None means KVQ_PARAM_GROUPS
        (JSON) from the environment (unset or empty: off).  Whether a pattern matches a parameter is checked by the constructor, which
        knows the names.  lr_scale 0 is allowed and does NOT freeze a group: its moments still move."""
        if v is None and env:
            import json
            v = TrainEngine._env_value("KVQ_PARAM_GROUPS", json.loads, "a JSON list of groups")
        if v is None:
            return None
        if not isinstance(v, (list, tuple)):
            raise KvqError(f"TrainEngine: param_groups must be None or a list of dicts, got {v!r}")
        if len(v) > MAX_PARAM_GROUPS:
            raise KvqError(f"TrainEngine: param_groups holds {len(v)} groups; at most {MAX_PARAM_GROUPS} beside the default group")
        out = []
        for j, g in enumerate(v):
            if not isinstance(g, dict) or "match" not in g or set(g) - {"match", "lr_scale", "weight_decay"}:
                raise KvqError(f"TrainEngine: param_groups[{j}] must be a dict with \"match\" and optionally \"lr_scale\", "
                               f"\"weight_decay\", got {g!r}")
            pats = [g["match"]] if isinstance(g["match"], str) else g["match"]
            if not isinstance(pats, (list, tuple)) or not pats or not all(isinstance(p, str) and p for p in pats):
                raise KvqError(f"TrainEngine: param_groups[{j}][\"match\"] must be a pattern or a non-empty list of patterns, got {g['match']!r}")
            vals = {}
            for key, default in (("lr_scale", 1.0), ("weight_decay", None)):
                x = g.get(key, default)
                if x is not None and (isinstance(x, bool) or not isinstance(x, (int, float)) or not 0 <= x < math.inf):
                    raise KvqError(f"TrainEngine: param_groups[{j}][{key!r}] must be a finite float >= 0, got {x!r}")
                vals[key] = None if x is None else float(x)
            out.append(dict(match=list(pats), **vals))
        return out

    @staticmethod
    def check_decoupled_weight_decay(v, env=False):
        """The bool a TrainEngine(decoupled_weight_decay=...) accepts (False: off, the coupled L2 term); env: None means KVQ_DECOUPLED_WD
        (0 / 1) from the environment."""
        if v is None and env and os.environ.get("KVQ_DECOUPLED_WD", "") != "":
            s = os.environ["KVQ_DECOUPLED_WD"]
            if s not in ("0", "1"):
                raise KvqError(f"TrainEngine: KVQ_DECOUPLED_WD (decoupled_weight_decay) must be 0 or 1, got {s!r}")
            v = s == "1"
        if v is None:
            return False
        if not isinstance(v, bool):
            raise KvqError(f"TrainEngine: decoupled_weight_decay must be None, False or True, got {v!r}")
        return v

    @staticmethod
    def check_lr_warmup_steps(v, env=False):
        """The int >= 0 a TrainEngine(lr_warmup_steps=...) accepts (0: off); env: None means KVQ_LR_WARMUP_STEPS."""
        if v is None and env:
            v = TrainEngine._env_value("KVQ_LR_WARMUP_STEPS", int, "an integer >= 0")
        if v is None:
            return 0
        if isinstance(v, bool) or not isinstance(v, int) or v < 0:
            raise KvqError(f"TrainEngine: lr_warmup_steps must be None or an integer >= 0, got {v!r}")
        return v

    @staticmethod
    def check_lr_decay(v, env=False):
        """None (off), "linear" or "cosine"; "none" means off; env: None means KVQ_LR_DECAY."""
        if v is None and env:
            v = TrainEngine._env_value("KVQ_LR_DECAY", str, "none, linear or cosine")
        if v is None or v == "none":
            return None
        if v not in ("linear", "cosine"):
            raise KvqError(f"TrainEngine: lr_decay must be None, \"none\", \"linear\" or \"cosine\", got {v!r}")
        return v

    @staticmethod
    def check_lr_total_steps(v, env=False):
        """None, or the int >= 1 a TrainEngine(lr_total_steps=...) accepts; env: None means KVQ_LR_TOTAL_STEPS."""
        if v is None and env:
            v = TrainEngine._env_value("KVQ_LR_TOTAL_STEPS", int, "an integer >= 1")
        if v is None:
            return None
        if isinstance(v, bool) or not isinstance(v, int) or v < 1:
            raise KvqError(f"TrainEngine: lr_total_steps must be None or an integer >= 1, got {v!r}")
        return v

    @staticmethod
    def check_lr_min_ratio(v, env=False):
        """None, or the float in [0, 1] a TrainEngine(lr_min_ratio=...) accepts; env: None means KVQ_LR_MIN_RATIO."""
        if v is None and env:
            v = TrainEngine._env_value("KVQ_LR_MIN_RATIO", float, "a float in [0, 1]")
        if v is None:
            return None
        if isinstance(v, bool) or not isinstance(v, (int, float)) or not 0 <= v <= 1:
            raise KvqError(f"TrainEngine: lr_min_ratio must be None or a float in [0, 1], got {v!r}")
        return float(v)

    @staticmethod
    def check_lr_schedule(warmup_steps, decay, total_steps, min_ratio):
        """The four checked schedule options together: None when no warm-up and no decay is asked for, else the tuple
        (warmup_steps, "none" | "linear" | "cosine", total_steps, min_ratio) of kvq_step_state_advance_sched.  A decay needs
        lr_total_steps > lr_warmup_steps; lr_total_steps / lr_min_ratio without a decay mean nothing and are refused."""
        if decay is None:
            if total_steps is not None or min_ratio is not None:
                raise KvqError("TrainEngine: lr_total_steps / lr_min_ratio without lr_decay (\"linear\" or \"cosine\")")
            return (warmup_steps, "none", 0, 0.0) if warmup_steps > 0 else None
        if total_steps is None or total_steps <= warmup_steps:
            raise KvqError(f"TrainEngine: lr_decay={decay!r} needs lr_total_steps > lr_warmup_steps, got {total_steps!r} and {warmup_steps!r}")
        return (warmup_steps, decay, total_steps, 0.0 if min_ratio is None else min_ratio)

    def param_names(self):
        """Every name a param_groups pattern is matched against: the flat buffer's entries in buffer order, then the parameters
        outside it (vq.codebook; vq.proj.weight, vq.proj.bias, vq.embed.weight of a Gumbel quantiser)."""
        return list(self.flat.seg) + list(self._aux_names)

    def param_group_of(self, name):
        """The group (0 = the default group) the parameter `name` is updated under."""
        if name not in self.flat.seg and name not in self._aux_names:
            raise KvqError(f"TrainEngine.param_group_of: no parameter named {name!r} (param_names() lists them)")
        return self._pg["group_of"][name] if self._pg is not None else 0

    def param_group_table(self):
        """One dict per group, group 0 first: group, match, lr_scale, weight_decay (resolved), names (members), elements (their
        parameter elements, frozen ones included).  Without param_groups: the one default group."""
        numel = {n: int(c) for n, (_, c, _) in self.flat.seg.items()}
        if self.has_vq and self.vq_kind != "GumbelQuantizer":
            numel["vq.codebook"] = self.E.numel()
        elif self.has_vq:
            gq = self.model.vector_quantizer
            numel.update({"vq.proj.weight": gq.proj.weight.numel(), "vq.proj.bias": gq.proj.bias.numel(),
                          "vq.embed.weight": gq.embed.weight.numel()})
        table = self._pg["table"] if self._pg is not None else \
            [dict(group=0, match=[], lr_scale=1.0, weight_decay=float(self.wd), names=self.param_names())]
        return [dict(group=g["group"], match=list(g["match"]), lr_scale=g["lr_scale"], weight_decay=g["weight_decay"],
                     names=len(g["names"]), elements=sum(numel[n] for n in g["names"])) for g in table]

    @property
    def weight_ema_updates(self):
        """Updates the average has taken so far (weight_ema only, 0 otherwise; synchronises).  A skipped step applies none."""
        return nnops.read_weight_ema_state(self._wema_state)[0] if self._wema_state is not None else 0

    def _wema_pairs(self):
        """(parameters, average, bf16 shadow | None) of everything that is averaged: the trainable ranges of the flat buffer, then
        the aux parameters Adam owns.  Views of fixed storage: what a captured launch or a swap addresses never moves."""
        fl = self.flat
        for (a, b) in fl.ranges:
            yield fl.master[a:b], fl.ema[a:b], (fl.shadow[a:b] if fl.shadow is not fl.master else None)
        for x in self.aux:
            if x["p"].requires_grad:
                yield x["p"].data.view(-1), x["ema"].view(-1), None

    def _weight_ema_update(self):
        """weight_ema, behind the step's last write to a parameter (Adam, the revived codebook rows): one update launch per range and
        per aux parameter, then the count moves.  Gated by the gradient guard like the Adam launches in front of it."""
        if self.weight_ema is None:
            return
        for p, ema, _ in self._wema_pairs():
            nnops.weight_ema_update(p, ema, self._wema_state, self.weight_ema, guard=self._guard)
        nnops.weight_ema_advance(self._wema_state, self.weight_ema, guard=self._guard)

    def _wema_refuse(self, what):
        if self._wema_applied:
            raise KvqError(f"TrainEngine.{what}: called inside weight_ema_applied() -- the parameters hold the average, the master "
                           f"weights sit in the average's buffer; leave the scope first")

    def _wema_swap(self):
        with torch.no_grad():
            for p, ema, shadow in self._wema_pairs():
                nnops.weight_ema_swap(p, ema, shadow=shadow)
        self._distrust_codebook_pack()         # the codebook changed under its pack: the next quantiser call repacks it

    @contextlib.contextmanager
    def weight_ema_applied(self):
        """Evaluate under the average: on entry every averaged range and aux parameter changes places with its average
        (kvq_weight_ema_swap, which also writes the bf16 shadow), on exit they change back -- exactly, bit for bit.  No address moves
        (captured steps stay valid) and no tensor version is bumped.  Inside, model.state_dict(), eval_step, forward_logits, encode /
        decode and attention_maps see the averaged weights; whatever would train on them, or save / load the engine's state, raises.
        Before the first update there is nothing to apply: nothing is swapped (the scope still refuses what it refuses)."""
        if self.weight_ema is None:
            raise KvqError("TrainEngine.weight_ema_applied: the engine keeps no average (weight_ema / KVQ_WEIGHT_EMA is off)")
        self._wema_refuse("weight_ema_applied")
        if self._cap is not None or self._in_fb:
            raise KvqError("TrainEngine.weight_ema_applied: called inside a step")
        swap = self.weight_ema_updates > 0
        self._wema_applied = True
        try:
            if swap:
                self._wema_swap()
            yield self
        finally:
            try:
                if swap:
                    self._wema_swap()
            finally:
                self._wema_applied = False

    @property
    def skipped_steps(self):
        """Optimiser steps skipped so far because their gradient was not finite (max_grad_norm only; synchronises)."""
        return nnops.read_grad_guard(self._guard)["skipped"] if self._guard is not None else 0

    def _gn_pieces(self, lo, hi):
        """Sum-of-squares launches over the parameter elements of the flat gradient inside [lo, hi): one per contiguous piece, each
        into the next kvq_grad_sumsq_partials() slots of the step's partials buffer."""
        grad, P = self._grad_src(), self._gn_P
        for (a, b) in self.flat.pieces:
            a, b = max(a, lo), min(b, hi)
            if a < b:
                nnops.grad_sumsq_partial(grad[a:b], self._gn_partials[self._gn_slot * P:(self._gn_slot + 1) * P])
                self._gn_slot += 1

    def _gn_begin(self, cut):
        """Size the partials buffer for this step's launches (the pieces, one more where `cut` splits one, the aux gradients)."""
        fl = self.flat
        n = sum(1 for (a, b) in fl.pieces if a < cut) + sum(1 for (a, b) in fl.pieces if b > cut) \
            + sum(1 for x in self.aux if x["p"].requires_grad)
        if n == 0:
            raise KvqError("TrainEngine: max_grad_norm on a model without a trainable parameter")
        if self._gn_partials is None or self._gn_partials.numel() != n * self._gn_P:
            if self._cap is not None:
                raise KvqError("TrainEngine: the gradient-norm partials buffer changed size inside a captured step")
            self._gn_partials = torch.zeros(n * self._gn_P, dtype=torch.float64, device=self.dev)
        self._gn_slot = 0

    def _gn_finish(self):
        """The aux gradients' partials, then the guard: norm, clipping coefficient, skip flag -- all on the device."""
        P = self._gn_P
        for x in self.aux:
            if x["p"].requires_grad:
                nnops.grad_sumsq_partial(x[self._aux_src].view(-1), self._gn_partials[self._gn_slot * P:(self._gn_slot + 1) * P])
                self._gn_slot += 1
        assert self._gn_slot * P == self._gn_partials.numel(), (self._gn_slot, self._gn_partials.numel())
        nnops.grad_guard_finalize(self._gn_partials, self.max_grad_norm, self._guard)

    def _grad_src(self):
        """What the optimiser reads as the flat gradient: the buffer backward wrote, or with grad_accum > 1 the f32 mean."""
        return self.flat.acc if self.grad_accum > 1 else self.flat.grad

    @property
    def _aux_src(self):
        return "acc" if self.grad_accum > 1 else "g"

    def _accumulate(self):
        """grad_accum > 1, behind backward (the queued reductions and weight gradients have been launched): the flat gradient of
        every trainable range, then the aux gradients, into their accumulators -- store, add, or add and average, as the device's
        position inside the cycle says."""
        fl, A = self.flat, self.grad_accum
        for (a, b) in fl.ranges:
            nnops.grad_accumulate(fl.grad[a:b], fl.acc[a:b], self._acc_state, A)
        for x in self.aux:
            if x["p"].requires_grad:
                nnops.grad_accumulate(x["g"].view(-1), x["acc"].view(-1), self._acc_state, A)

    def _finish_step(self, final=True):
        """What follows forward and backward in a train_step.  grad_accum 1: the optimiser.  grad_accum > 1: accumulate, the
        optimiser on the cycle's last micro-step (`final`), then the device's position moves on."""
        if self.grad_accum == 1:
            self.optimizer_step()
            return
        self._accumulate()
        if final:
            self.optimizer_step()
        nnops.accum_advance(self._acc_state, self.grad_accum)

    def _adam(self, p, g, m, v, vmax, shadow, flat_range=None, aux_name=None):
        """The engine's one Adam launch: elements [a, b) = flat_range of the flat buffer, or the aux parameter aux_name."""
        b1, b2 = self.betas
        fp8 = None
        if flat_range is not None and self.fp8 and self._w8_in_adam:
            a, b = flat_range
            if a % 8 or b % 8:           # (segments and chunk cuts are multiples of 16: cannot happen; a silent fallback would
                raise KvqError(f"TrainEngine: Adam range [{a}, {b}) is not 8-aligned")       # leave the fp8 mirror stale)
            fp8 = (*self._w8_adam, a)    # the update also writes the fp8 mirror of the GEMM weights in [a, b) (scales of the last refresh)
        if self._pg is None:
            nnops.adam_step_dev(p, g, m, v, self._state, b1, b2, self.eps, self.wd, vmax=vmax, shadow=shadow, guard=self._guard, fp8=fp8)
            return
        # parameter groups: still ONE launch.  An aux parameter, or a range whose blocks share a group j, passes no block table (the
        # work of adam_step_dev); any other range looks its groups up per 16-element block of the flat buffer, indexed from element a.
        pg = self._pg
        if aux_name is not None:
            j = pg["group_of"][aux_name]
        else:
            if flat_range not in pg["range_group"]:
                pg["range_group"][flat_range] = range_group(pg["blocks_host"], *flat_range)
            j = pg["range_group"][flat_range]
        one = slice(None) if j is None else slice(j, j + 1)
        nnops.adam_step_grouped(p, g, m, v, self._state, b1, b2, self.eps, self.wd, vmax=vmax, shadow=shadow, guard=self._guard,
                                block_group=pg["blocks"] if j is None else None, first_element=0 if flat_range is None else flat_range[0],
                                group_lr_scale=pg["scale"][one], group_wd=pg["wd"][one],
                                n_groups=len(pg["table"]) if j is None else 1, decoupled=self.decoupled_wd)

    def _adam_ranges(self, lo, hi):
        fl = self.flat
        grad = self._grad_src()
        for (a, b) in fl.ranges:
            a, b = max(a, lo), min(b, hi)
            if a < b:
                self._adam(fl.master[a:b], grad[a:b], fl.m[a:b], fl.v[a:b], fl.vmax[a:b] if fl.vmax is not None else None,
                           fl.shadow[a:b] if fl.shadow is not fl.master else None, flat_range=(a, b))

    def optimizer_step(self):
        self._wema_refuse("optimizer_step")
        fl = self.flat
        b1, b2 = self.betas
        cut = 0
        if self._dp:
            cut = self._pending_hi                    # [0, cut) has not been sent yet (embedding gradients)
            self._eager(lambda: self._exchange_head(cut))
            self._pending_hi = fl.n
        self._wg_done_lo = fl.n
        if self.vq_ema:          # the codebook follows the EMA of its assigned encoder outputs (backward has used the old one by now)
            self._eager(self._ema_step)
        self._step_host += 1
        if self._guard is not None:
            # max_grad_norm: every Adam launch waits for the norm of the WHOLE (averaged) gradient.  Multi-GPU: the tail [cut, n) is
            # reduced while the head is still being exchanged, the head, the aux gradients and the guard behind _exchange_tail -- Adam
            # no longer overlaps the head's all-reduce.  A skipped step still advances the step state.
            self._gn_begin(cut)
            self._gn_pieces(cut, fl.n)
            if self._dp:
                self._eager(self._exchange_tail)
                self._gn_pieces(0, cut)
            self._gn_finish()
            self._advance_state()
            self._adam_ranges(0, fl.n)
            self._adam_aux()
            self._revive_apply()
            self._weight_ema_update()
            self._after_update()
            return
        # step += 1, lr after the milestones, bias corrections: computed on the device, read there by the Adam kernels
        self._advance_state()
        self._adam_ranges(cut, fl.n)                  # multi-GPU: runs while the head of the buffer is still being reduced
        if self._dp:
            self._eager(self._exchange_tail)
            self._adam_ranges(0, cut)
        self._adam_aux()
        self._revive_apply()
        self._weight_ema_update()
        self._after_update()

    def _advance_state(self):
        """step += 1, lr and bias corrections of the step on the device; without a schedule option the neutral schedule."""
        W, kind, T, r = self.lr_schedule or (0, "none", 0, 0.0)
        nnops.step_state_advance_sched(self._state, self.lr, self.gamma, self.milestones, *self.betas, warmup_steps=W,
                                       decay_kind=nnops.LR_DECAY_KINDS[kind], total_steps=T, min_ratio=r)

    def _adam_aux(self):
        for a in self.aux:
            if a["p"].requires_grad:
                self._adam(a["p"].data.view(-1), a[self._aux_src].view(-1), a["m"].view(-1), a["v"].view(-1),
                           a["vmax"].view(-1) if a["vmax"] is not None else None, None, aux_name=a["name"])

    def _after_update(self):
        if self.vq_kind in ("VectorQuantizer", "MultiVectorQuantizer") and (self.E.requires_grad or self.revive_after is not None):
            self._repack_codebook()
        if self.fp8:
            self._fp8_quantize_weights(in_step=True)

    def _versions(self):
        return sum(p._version for p in self.param_of.values())

    def refresh_if_params_changed(self):
        """Parameters written from outside (an optimiser step of the autograd path, load_state_dict) since the bf16 shadow was
        last refreshed: refresh it.  The engine's own Adam kernel keeps the shadow current and does not bump tensor versions."""
        v = self._versions()
        if v != self._param_versions:
            self.flat.refresh_shadow()
            if self.fp8:
                self._fp8_quantize_weights()
            self._param_versions = v

    def sync_from_model(self):
        """Call after the model's parameters were written from outside (load_state_dict, manual init): refreshes the bf16
        shadow weights the GEMMs read.  (The f32 master buffer IS the parameters' storage, nothing to copy there.)"""
        self.flat.refresh_shadow()
        if self.fp8:
            self._fp8_quantize_weights()
        self._distrust_codebook_pack()         # the codebook pack is rebuilt by the next quantiser call

    # ------------------------------------------------------------------------------------------------------------
    # resumable training: everything that makes step n + 1 follow step n, as plain CPU data.  Off the step's
    # path: an engine on which neither method is called allocates nothing and launches nothing for them.
    # ------------------------------------------------------------------------------------------------------------
    STATE_FORMAT = 1

    def state_fingerprint(self) -> dict:
        """Everything that changes the bits of a step or the meaning of a buffer, as plain Python values: a state is loaded only
        into an engine whose fingerprint equals the stored one (load_state_dict refuses, it does not convert)."""
        fl = self.flat
        scope = False if not self.fp8 else ("fused" if self._fp8_fused else ("all" if self._fp8_all else "wide"))
        return {
            "layout": [[name, int(o), int(n), bool(fl.trainable[name])] for name, (o, n, _) in fl.seg.items()],
            "flat_n": int(fl.n),
            "dtype": str(self.dtype),
            "lr": float(self.lr), "betas": [float(b) for b in self.betas], "eps": float(self.eps), "weight_decay": float(self.wd),
            "amsgrad": bool(fl._amsgrad), "milestones": [int(m) for m in self.milestones], "gamma": float(self.gamma),
            "w_recon": self.w_recon, "w_vq": self.w_vq, "seed": self.seed,
            "grad_accum": int(self.grad_accum), "max_grad_norm": self.max_grad_norm, "revive_after": self.revive_after,
            "vq_kind": self.vq_kind, "G": int(self.G), "K": getattr(self, "K", None), "Dg": getattr(self, "Dg", None),
            "vq_ema": bool(self.vq_ema),
            "aux": [[list(a["p"].shape), bool(a["p"].requires_grad)] for a in self.aux],
            "fp8": scope, "fp8_backward": bool(self.fp8_backward),
            "w8_period": int(self._w8_period) if self.fp8 else None, "w8_in_adam": bool(self._w8_in_adam) if self.fp8 else None,
            "w8_keys": list(self._w8_index) if self.fp8 else [],
            "world": int(self.world),
            **({"weight_ema": float(self.weight_ema)} if self.weight_ema is not None else {}),     # off: exactly the keys of before
            **({"loss_ignore_pad": True} if self.loss_ignore_pad else {}),
            **({"param_groups": [[list(g["match"]), g["lr_scale"], g["weight_decay"], list(g["names"])] for g in self._pg["table"]]}
               if self._pg_spec is not None else {}),
            **({"decoupled_weight_decay": True} if self.decoupled_wd else {}),
            **({"lr_schedule": list(self.lr_schedule)} if self.lr_schedule is not None else {}),
        }

    def _state_slots(self, present) -> dict:
        """{path: (destination getter, dtype, numel, required)} of every tensor a state may hold for THIS engine.  A getter is
        called only when the copy happens: the lazily allocated buffers (moments, accumulator) stay unallocated until then.
        present(path): whether the state at hand holds that entry (decides the optional ones)."""
        fl, f32, i64 = self.flat, torch.float32, torch.int64
        slots = {"flat.master": (lambda: fl.master, f32, fl.n, True)}
        moments = present("flat.m") or present("flat.v")          # all of them or (a state from before the first step) none
        for k in ("m", "v") + (("vmax",) if fl._amsgrad else ()):
            slots["flat." + k] = ((lambda k=k: getattr(fl, k)), f32, fl.n, moments)
        pending = self.grad_accum > 1 and present("host.accum_pending")
        if self.grad_accum > 1:
            slots["flat.acc"] = (lambda: fl.acc, f32, fl.n, pending)
        if self.weight_ema is not None:           # (absent in a state from before the first update, like the moments)
            slots["flat.ema"] = (lambda: fl.ema, f32, fl.n, present("flat.ema"))
            slots["structs.weight_ema"] = (lambda: self._wema_state, i64, 2, True)
        for i, a in enumerate(self.aux):
            for k in ("p", "m", "v") + (("vmax",) if a["vmax"] is not None else ()) + (("acc",) if "acc" in a else ()) \
                    + (("ema",) if "ema" in a else ()):
                get = (lambda a=a: a["p"].data) if k == "p" else (lambda a=a, k=k: a[k])
                slots[f"aux.{i}.{k}"] = (get, a["p"].dtype, a["p"].numel(), pending if k == "acc" else True)
        slots["structs.state"] = (lambda: self._state, i64, 3, True)
        if self._acc_state is not None:
            slots["structs.acc_state"] = (lambda: self._acc_state, i64, 2, True)
        if self._guard is not None:
            slots["structs.guard"] = (lambda: self._guard, i64, 4, True)
        if self.revive_after is not None:
            slots["structs.revive_idle"] = (lambda: self._rv_idle, torch.int32, self.G * self.K, True)
            slots["structs.revive_counter"] = (lambda: self._rv_counter, i64, 2, True)
        if self.vq_kind in ("VectorQuantizer", "MultiVectorQuantizer") and not self.E.requires_grad:
            # a codebook Adam does not own (EMA, a frozen mode) is in neither the flat buffer nor aux: here, so that the state is whole
            slots["structs.codebook"] = (lambda: self.E.data, self.E.dtype, self.E.numel(), True)
        if self.vq_ema:          # likewise the EMA statistics, buffers of the module
            vq = self.model.vector_quantizer
            slots["structs.ema_n"] = (lambda: vq.ema_n, vq.ema_n.dtype, vq.ema_n.numel(), True)
            slots["structs.ema_m"] = (lambda: vq.ema_m, vq.ema_m.dtype, vq.ema_m.numel(), True)
        if self.fp8:
            slots["fp8.w8"] = (lambda: self._w8, torch.uint8, fl.n, True)
            slots["fp8.w8_amax"] = (lambda: self._w8_amax, f32, self._w8_amax.numel(), True)
            slots["fp8.w8_scale"] = (lambda: self._w8_scale, f32, self._w8_scale.numel(), True)
            slots["fp8.a8_state"] = (lambda: self._a8_state, f32, self._a8_state.numel(), True)
            if self.fp8_backward:
                slots["fp8.g8_state"] = (lambda: self._g8_state, f32, self._g8_state.numel(), True)
        return slots

    def state_dict(self) -> dict:
        """The engine's full training state between two train_step calls (an open accumulation cycle included), as a plain dict of
        CPU tensors and Python scalars / lists / dicts: it survives torch.save and torch.load(weights_only=True).  Device-to-host
        copies only -- nothing that writes is enqueued, the bits of every later step are what they would have been.  The small
        device structs travel as raw words, so a state is tied to their layout in include/kvq.h (kvq_version).  flat.grad and
        flat.shadow are not state (every backward rewrites the first, refresh_shadow() rebuilds the second), nor are the graphs."""
        fl = self.flat
        self._wema_refuse("state_dict")
        if self._cap is not None or self._in_fb:
            raise KvqError("TrainEngine.state_dict: called inside a step")
        pending = self._accum_host > 0
        flat = {"master": fl.master}
        for k in ("m", "v", "vmax"):
            if getattr(fl, "_" + k) is not None:
                flat[k] = getattr(fl, "_" + k)
        if pending:
            flat["acc"] = fl.acc
        if fl._ema is not None:
            flat["ema"] = fl._ema
        aux = []
        for a in self.aux:
            d = {"p": a["p"].data, "m": a["m"], "v": a["v"]}
            if a["vmax"] is not None:
                d["vmax"] = a["vmax"]
            if pending and "acc" in a:
                d["acc"] = a["acc"]
            if "ema" in a:
                d["ema"] = a["ema"]
            aux.append(d)
        structs = {"state": self._state}
        if self._acc_state is not None:
            structs["acc_state"] = self._acc_state
        if self._guard is not None:
            structs["guard"] = self._guard
        if self._wema_state is not None:
            structs["weight_ema"] = self._wema_state
        if self.revive_after is not None:
            structs["revive_idle"], structs["revive_counter"] = self._rv_idle, self._rv_counter
        if self.vq_kind in ("VectorQuantizer", "MultiVectorQuantizer") and not self.E.requires_grad:
            structs["codebook"] = self.E.data
        if self.vq_ema:
            structs["ema_n"], structs["ema_m"] = self.model.vector_quantizer.ema_n, self.model.vector_quantizer.ema_m
        cpu = lambda d: {k: v.detach().cpu() for k, v in d.items()}
        out = {"format": self.STATE_FORMAT, "kvq_version": int(lib().kvq_version()), "fingerprint": self.state_fingerprint(),
               "flat": cpu(flat), "aux": [cpu(d) for d in aux], "structs": cpu(structs),
               "host": {"step": int(self._step_host), "accum_pending": int(self._accum_host), "grads_are_mean": bool(self._grads_are_mean)}}
        if self.fp8:
            f8 = {"w8": self._w8, "w8_amax": self._w8_amax, "w8_scale": self._w8_scale, "a8_state": self._a8_state}
            if self.fp8_backward:
                f8["g8_state"] = self._g8_state
            out["fp8"] = cpu(f8)
            if self.fp8_backward:
                out["fp8"]["g8_ready"], out["fp8"]["g8_live"] = bool(self._g8_ready), sorted(self._g8_live)
        return out

    @staticmethod
    def _state_entry(state, path):
        """state["a"]["b"] / state["aux"][i]["k"] for path "a.b" / "aux.i.k"; None when it is not there."""
        node = state
        for part in path.split("."):
            if isinstance(node, dict):
                node = node.get(part)
            elif isinstance(node, (list, tuple)) and part.isdigit() and int(part) < len(node):
                node = node[int(part)]
            else:
                return None
            if node is None:
                return None
        return node

    def load_state_dict(self, state) -> None:
        """Continue where the engine that wrote `state` (state_dict()) stood.  First every check -- format, kvq_version, the whole
        fingerprint, presence / dtype / size of every entry -- and a KvqError naming each differing key with both values; a refused
        load has written nothing.  Then copies INTO the existing buffers: no attribute a captured graph may hold the address of is
        rebound, an engine that replays graphs keeps replaying them.  Not sync_from_model(): that would re-quantise the fp8 weights
        with fresh scales in the middle of a scale period."""
        self._wema_refuse("load_state_dict")
        if self._cap is not None or self._in_fb:
            raise KvqError("TrainEngine.load_state_dict: called inside a step")
        if not isinstance(state, dict):
            raise KvqError(f"TrainEngine.load_state_dict: a state_dict() is a dict, got {type(state).__name__}")
        short = lambda v: (lambda r: r if len(r) <= 120 else r[:117] + "...")(repr(v))
        bad = []
        for key, want in (("format", self.STATE_FORMAT), ("kvq_version", int(lib().kvq_version()))):
            if key not in state:
                bad.append(f"{key}: missing")
            elif state[key] != want or isinstance(state[key], bool):
                bad.append(f"{key}: state {short(state[key])}, engine {short(want)}")
        mine, theirs = self.state_fingerprint(), state.get("fingerprint")
        if not isinstance(theirs, dict):
            bad.append("fingerprint: missing")
        elif not bad:
            for key in sorted(set(mine) | set(theirs)):
                if key not in theirs or key not in mine:
                    bad.append(f"fingerprint.{key}: " + ("missing in the state" if key not in theirs else "unknown to this engine"))
                elif theirs[key] != mine[key]:
                    a, b = theirs[key], mine[key]
                    if key == "layout" and isinstance(a, list):          # the first entry that differs says more than two long lists
                        i = next((i for i, (x, y) in enumerate(zip(a, b)) if x != y), min(len(a), len(b)))
                        a = f"{len(a)} entries, [{i}] = {a[i] if i < len(a) else None}"
                        b = f"{len(b)} entries, [{i}] = {b[i] if i < len(b) else None}"
                    bad.append(f"fingerprint.{key}: state {short(a)}, engine {short(b)}")
        if bad:
            raise KvqError("TrainEngine.load_state_dict: this state does not belong to this engine -- " + "; ".join(bad))
        host = state.get("host")
        for key, typ in (("step", int), ("accum_pending", int), ("grads_are_mean", bool)):
            if not isinstance(host, dict) or not isinstance(host.get(key), typ):
                bad.append(f"host.{key}: missing")
        if not bad and not 0 <= host["accum_pending"] < self.grad_accum:
            bad.append(f"host.accum_pending: state {host['accum_pending']}, engine has cycles of {self.grad_accum}")
        present = lambda path: bool(self._state_entry(state, path)) if path.startswith("host.") else self._state_entry(state, path) is not None
        slots = self._state_slots(present)
        plan = []
        for path, (get, dtype, numel, required) in slots.items():
            t = self._state_entry(state, path)
            if t is None:
                if required:
                    bad.append(f"{path}: missing")
                continue
            if not torch.is_tensor(t) or t.dtype != dtype or t.numel() != numel:
                got = f"{t.dtype} x {t.numel()}" if torch.is_tensor(t) else type(t).__name__
                bad.append(f"{path}: state {got}, engine {dtype} x {numel}")
                continue
            plan.append((get, t))
        if self.fp8_backward:
            f8 = state.get("fp8") if isinstance(state.get("fp8"), dict) else {}
            if not isinstance(f8.get("g8_ready"), bool):
                bad.append("fp8.g8_ready: missing")
            live = f8.get("g8_live")
            if not isinstance(live, list) or any(k not in self._g8_index for k in live):
                bad.append(f"fp8.g8_live: state {short(live)}, engine knows the sites {short(sorted(self._g8_index))}")
        if bad:
            raise KvqError("TrainEngine.load_state_dict: this state does not belong to this engine -- " + "; ".join(bad))
        # ---- from here on the engine is written
        fl = self.flat
        with torch.no_grad():
            for get, t in plan:
                dst = get()
                dst.copy_(t.reshape(dst.shape))
            if present("flat.m") is False and fl.optimizer_state_allocated():       # a state from before the first step: moments restart
                for k in ("_m", "_v", "_vmax"):
                    if getattr(fl, k) is not None:
                        getattr(fl, k).zero_()
        self._step_host, self._accum_host = int(host["step"]), int(host["accum_pending"])
        self._grads_are_mean = bool(host["grads_are_mean"])
        self._rv_pending = False
        fl.refresh_shadow()
        self._distrust_codebook_pack()                 # the next quantiser call repacks the codebook
        if self.fp8_backward:
            ready, live = bool(state["fp8"]["g8_ready"]), set(state["fp8"]["g8_live"])
            if (ready, live) != (self._g8_ready, self._g8_live):
                # another set of live sites: another per-step transpose table -- chains captured with the old one are not this state's
                self._graphs.clear()
                self._eager_seen.clear()
                self._g8_ready, self._g8_live = ready, live
                self._fp8_transpose_table([t for t in self._w8t_sites if t[0] in live] if ready else self._w8t_sites)
            self._fp8_transpose_weights()
        # the in-place writes (and a model.load_state_dict before this call) bumped tensor versions: not a write from outside
        self._param_versions = self._versions()

    @staticmethod
    def supports(model, seq_len: int) -> bool:
        """The engine covers BERT-shaped models with 64-wide heads and sentences of at most 32 tokens (the benchmarked kernels;
        up to 128 in bf16 through the blocked attention kernels)."""
        cfg = model.encoder.config
        kind = type(getattr(model, "vector_quantizer", None)).__name__
        s_max = 128 if getattr(model, "compute_dtype", torch.float32) == torch.bfloat16 else 32
        return kind in _QUANTIZERS + ("NoneType",) and cfg.hidden_size // cfg.num_attention_heads == 64 and seq_len <= s_max \
            and seq_len <= cfg.max_position_embeddings \
            and cfg.hidden_size % 32 == 0 and next(model.parameters()).is_cuda

    def prepare_batch(self, input_ids):
        """What the word-embedding gradient needs besides the ids: the tokens in a STABLE order by id (sorted_ids, perm), pad
        tokens filed under id -1 (nn.Embedding(padding_idx) of BertEmbeddings, modeling_bert.py:60: the pad row receives no
        gradient; kvq_embed_grad ignores negative ids).  Part of building a batch -- hand the result to train_step(prepared=...)
        (dsentences.token_cache does) and the step itself contains no sort; without it the engine sorts before the step."""
        flat_ids = input_ids.reshape(-1)
        if self._pad_idx is not None:
            flat_ids = torch.where(flat_ids == self._pad_idx, torch.full_like(flat_ids, -1), flat_ids)
        srt, perm = torch.sort(flat_ids, stable=True)
        return srt, perm

    def pack_batch(self, input_ids, attention_mask, dec_ids=None, dec_mask=None, target_ids=None):
        """ids | mask | sorted ids | order as ONE int64 tensor [4, B*S]: a replayed step then starts with one device copy.
        With the decoder's own input (a Bagon step): one flat tensor of 4*B*S + 5*B*Sd entries, the same four rows followed by
        the decoder's ids | mask | sorted ids | order | loss target (= the decoder ids unless target_ids is given)."""
        srt, perm = self.prepare_batch(input_ids)
        rows = [input_ids.reshape(-1), attention_mask.reshape(-1).to(torch.int64), srt, perm]
        if dec_ids is None:
            if dec_mask is not None or target_ids is not None:
                raise KvqError("TrainEngine.pack_batch: dec_mask / target_ids without dec_ids")
            return torch.stack(rows)
        dsrt, dperm = self.prepare_batch(dec_ids)
        rows += [dec_ids.reshape(-1), dec_mask.reshape(-1).to(torch.int64), dsrt, dperm,
                 (dec_ids if target_ids is None else target_ids).reshape(-1)]
        return torch.cat(rows)

    @staticmethod
    def unpack_batch(pack, enc_shape, dec_shape=None):
        """Views into a pack_batch() tensor: (ids, mask, sorted ids, order, None | (dec ids, dec mask, sorted, order, target))."""
        flat = pack.reshape(-1)
        N = enc_shape[0] * enc_shape[1]
        Nd = dec_shape[0] * dec_shape[1] if dec_shape is not None else 0
        if flat.numel() != 4 * N + 5 * Nd or flat.dtype != torch.int64:
            raise KvqError(f"TrainEngine: a packed batch of {flat.numel()} {flat.dtype} entries does not fit ids {tuple(enc_shape)}"
                           + (f" + decoder ids {tuple(dec_shape)}" if dec_shape is not None else "")
                           + " (pack_batch() of the same call's ids)")
        r = [flat[i * N:(i + 1) * N] for i in range(4)]
        dec = None
        if dec_shape is not None:
            d = [flat[4 * N + i * Nd: 4 * N + (i + 1) * Nd] for i in range(5)]
            dec = (d[0].view(dec_shape), d[1].view(dec_shape), d[2], d[3], d[4].view(dec_shape))
        return r[0].view(enc_shape), r[1].view(enc_shape), r[2], r[3], dec

    def _normalise_prepared(self, prepared, input_ids, dec_ids=None, check_ids=False):
        """`prepared` of train_step() in one form: dict(pack = the whole batch as pack_batch() laid it out | None,
        enc = (sorted ids, order) | None, dec = likewise for the decoder's ids).  Accepted: None; prepare_batch()'s tuple (the
        encoder side); a dict(enc=tuple, dec=tuple); a pack_batch() tensor.  A pack is authoritative: the step reads ids, masks
        and target from it (eagerly and on replay alike); check_ids compares them with the ids of the call (a device sync:
        done on the first, eager steps of a batch shape)."""
        none = dict(pack=None, enc=None, dec=None)
        if prepared is None:
            return none
        def pair(t, ids, what):
            if t is None:
                return None
            if not isinstance(t, (tuple, list)) or len(t) != 2 or any(not torch.is_tensor(x) or x.numel() != ids.numel() or x.dtype != torch.int64
                                                                      for x in t):
                raise KvqError(f"TrainEngine: prepared {what} = (sorted ids, order) must be prepare_batch() of this call's {what} ids")
            return (t[0].reshape(-1), t[1].reshape(-1))
        if isinstance(prepared, dict):
            if prepared.get("dec") is not None and dec_ids is None:
                raise KvqError("TrainEngine: prepared holds a decoder side but the call passes no dec_ids")
            return dict(none, enc=pair(prepared.get("enc"), input_ids, "encoder"),
                        dec=pair(prepared.get("dec"), dec_ids, "decoder") if dec_ids is not None else None)
        if isinstance(prepared, (tuple, list)):
            return dict(none, enc=pair(prepared, input_ids, "encoder"))
        if not torch.is_tensor(prepared):
            raise KvqError(f"TrainEngine: prepared must be pack_batch()'s tensor or prepare_batch()'s tuple, got {type(prepared).__name__}")
        ids, mask, srt, perm, dec = self.unpack_batch(prepared, input_ids.shape, dec_ids.shape if dec_ids is not None else None)
        if check_ids and not (torch.equal(ids, input_ids) and (dec is None or torch.equal(dec[0], dec_ids))):
            raise KvqError("TrainEngine: the packed batch holds other ids than the ones passed to train_step()")
        return dict(pack=prepared.reshape(-1), enc=(srt, perm), dec=dec[2:4] if dec is not None else None, views=(ids, mask, dec))

    def _train_step_eager(self, input_ids, attention_mask, prep, dec=None):
        if prep["pack"] is not None:              # the pack is what a replayed step reads: the eager step reads the same tensors
            input_ids, attention_mask, dv = prep["views"]
            dec = (dv[0], dv[1], dv[4]) if dv is not None else None
        self._prepared = prep
        dkw = dict(dec_ids=dec[0], dec_mask=dec[1], target_ids=dec[2]) if dec is not None else {}
        try:
            out = self.forward_backward(input_ids, attention_mask, training=self.model.training, compute_grads=True, **dkw)
        finally:
            self._prepared = None
        final = self.finish_step()
        if self._guard is not None and final:  # copies: the guard state is rewritten by the next step
            out.update({k: v.clone() for k, v in self._guard_out.items()})
        if self.revive_after is not None and final:      # counter.last (its upper word is padding: 0), rewritten by the next step
            out["codes_revived"] = self._rv_counter[0].clone()
        if self.weight_ema is not None and final:
            out["weight_ema_decay"] = self._wema_out.clone()
        if self.lr_schedule is not None and final:
            out["lr"] = self._lr_out.clone()
        out["optimizer_step"] = final
        return out

    def _accum_final(self):
        """True when the micro-step about to run is the last of its cycle (always, with grad_accum 1)."""
        return self._accum_host == self.grad_accum - 1

    def _accum_note(self, final):
        """Host bookkeeping behind a finished micro-step (the device moved its own position: kvq_accum_advance)."""
        if self.grad_accum > 1:
            self._accum_host = 0 if final else self._accum_host + 1
            self._grads_are_mean = final

    def finish_step(self):
        """What train_step runs behind forward_backward(compute_grads=True), for callers that schedule the two halves themselves:
        the optimiser -- or, with grad_accum > 1, this micro-step's accumulation and the optimiser on the last one of a cycle.
        Returns whether the optimiser ran."""
        self._wema_refuse("finish_step")
        final = self._accum_final()
        self._finish_step(final)
        self._accum_note(final)
        return final

    def train_step(self, input_ids, attention_mask, prepared=None, dec_ids=None, dec_mask=None, target_ids=None):
        """One optimiser step -- with grad_accum = A > 1 one MICRO-step: forward, backward, the gradient added into the f32
        accumulator, and on every A-th call the optimiser on the mean of the A gradients (out["optimizer_step"] says whether it
        ran; grad_norm / grad_clip_coef / codes_revived appear only then).
        dec_ids / dec_mask / target_ids: the decoder's own input and the loss target of a Bagon step
        (models/bagon/Trainer.py:78-110; default: the autoencoding step, decoder input = target = input_ids).  prepared: see
        _normalise_prepared().  Once a batch shape has been seen twice the step is replayed from a chain of hipGraphs
        (_StepGraphs: the quantiser and, on multi-GPU runs, the RCCL all-reduces stay eager launches between the graphs); the
        host then issues a handful of launches per step instead of ~800.  KVQ_GRAPH=0 keeps every launch eager."""
        self._wema_refuse("train_step")
        if dec_ids is None and (dec_mask is not None or target_ids is not None):
            if target_ids is None:
                raise KvqError("TrainEngine.train_step: dec_mask without dec_ids")
            dec_ids, dec_mask = input_ids, attention_mask           # a separate target alone: the decoder still reads the encoder's ids
        dec = (dec_ids, dec_mask, target_ids) if dec_ids is not None else None
        shape_key = (tuple(input_ids.shape), bool(self.model.training), tuple(dec_ids.shape) if dec is not None else None)
        # grad_accum > 1: two chains per batch shape -- micro (forward, backward, accumulate, advance; whether it stores or adds is
        # decided on the device, so one chain serves positions 0 .. A-2) and final (the same plus the optimiser)
        final = self._accum_final()
        key = shape_key if self.grad_accum == 1 else shape_key + (final,)
        seen = self._eager_seen.get(key, 0)
        prep = self._normalise_prepared(prepared, input_ids, dec_ids, check_ids=seen < 2)
        if not self.use_graph:
            self._eager_seen[key] = seen + 1
            return self._train_step_eager(input_ids, attention_mask, prep, dec)
        g = self._graphs.get(key)
        if g is None:
            # warm the workspaces / GEMM plans eagerly first; few shapes only; fp8_backward: its calibration step is eager
            shapes = {k[:3] for k in self._graphs}             # the cap counts batch shapes, not chains
            if seen < 2 or (len(shapes) >= 4 and shape_key not in shapes) or (self.fp8_backward and not self._g8_ready):
                self._eager_seen[key] = seen + 1
                return self._train_step_eager(input_ids, attention_mask, prep, dec)
            try:
                if prep["pack"] is not None:
                    ids0, mask0, dv = prep["views"]
                    dec0 = (dv[0], dv[1], dv[4]) if dv is not None else None
                else:
                    ids0, mask0, dec0 = input_ids, attention_mask, dec
                g = self._graphs[key] = _StepGraphs(self, ids0, mask0, dec0, final=final)
            except Exception as e:                       # capture is an optimisation: never let it take a run down
                if os.environ.get("KVQ_GRAPH_STRICT", "0") == "1":      # (tests: a capture that fails is a failure)
                    self._abandon_capture()
                    raise
                import sys
                print(f"[kvq] hipGraph capture of the training step failed ({type(e).__name__}: {e}); "
                      f"continuing with eager launches", file=sys.stderr, flush=True)
                self._abandon_capture()
                return self._train_step_eager(input_ids, attention_mask, prep, dec)
        out = g.run(input_ids, attention_mask, prep, dec)
        self._accum_note(final)
        out["optimizer_step"] = final
        return out

    def _abandon_capture(self):
        """Leave a failed capture behind in a state from which eager steps can go on (same collectives, same order)."""
        self.use_graph, self._cap = False, None
        self._graphs.clear()
        try:
            torch.cuda.synchronize(self.dev)
        except Exception:
            pass
        if self._dp:
            try:
                self._settle(self._works)
                self._exchange_tail()
            except Exception:
                self._works, self._works_late = [], []
            self._pending_hi = self.flat.n
        self._wg_done_lo = self.flat.n
        self._red_items, self._red_keep = [], []
        self._wg_reset()

    def eval_step(self, input_ids, attention_mask, dec_ids=None, dec_mask=None, target_ids=None):
        return self.forward_backward(input_ids, attention_mask, training=False, compute_grads=False, dec_ids=dec_ids, dec_mask=dec_mask,
                                     target_ids=target_ids)
