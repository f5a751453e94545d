"""Bit-exact parity of the batched reductions (colsum_partial_kernel, reduce_batch_kernel in slab and tree mode, sum_slabs_kernel
of csrc/kvq_nn.hip) on integer operands.

Sources hold integers in [-8, 8] (exact in bf16 and f32) and counts stay <= 4096, so every partial sum in any order is an integer
below 2^24 and f32 accumulation is exact whatever grouping a kernel uses: an f32 destination must EQUAL the int64 reference, a bf16
destination must be its single RNE rounding, bit for bit.  The row counts walk every loop remainder (r + 12 < r1 / r < r1 in
colsum; p + 4 <= count / p < count in slab mode; p + 64 < count and p + 16 < count in tree mode) and both sides of each lane's
choice between vector and scalar access.  Every destination and partial buffer sits in a sentinel frame that must not change."""
import itertools

import pytest
import torch

import _pointwise_ref as R

pytestmark = pytest.mark.gpu

PAD = 64                      # frame elements on either side (keeps 16-byte alignment for both dtypes)
SENTINEL = 77.0
F32, BF16 = torch.float32, torch.bfloat16
SCALE_ACC = [(1.0, False), (0.5, True), (-2.0, True), (-2.0, False), (0.5, False), (1.0, True)]


@pytest.fixture(scope="module")
def ops():
    from kvq import _ffi, nnops
    _ffi.lib()
    assert torch.cuda.is_available()
    return nnops


class Framed:
    """A destination of n elements inside a sentinel frame; check() compares the frame with its snapshot."""

    def __init__(self, n, dtype, init=None):
        self.n = n
        self.buf = torch.full((n + 2 * PAD,), SENTINEL, dtype=dtype, device="cuda")
        self.view = self.buf[PAD:PAD + n]
        if init is not None:
            self.view.copy_(init.to(dtype))
        self.snap = self.buf.clone()

    def check(self, what):
        assert torch.equal(self.buf[:PAD], self.snap[:PAD]) and torch.equal(self.buf[PAD + self.n:], self.snap[PAD + self.n:]), \
            f"{what}: wrote outside its destination"


def _is_slab(src_ptr, dst_ptr, count, cols, ld):
    """reduce_is_slab of csrc/kvq_nn.hip: the test states which path a case is meant for and checks that it gets there."""
    return count <= 32 and cols % 8 == 0 and ld % 8 == 0 and src_ptr % 16 == 0 and dst_ptr % 16 == 0


def _tree_is_vec(src_ptr, cols, ld, itemsize):
    return cols % 4 == 0 and ld % 4 == 0 and src_ptr % (4 * itemsize) == 0


def _run_item(ops, count, cols, ld, sdt, ddt, scale, acc, seed, src_offset=0, expect=None):
    """One reduce_batch launch of one item; returns the number of wrong destination elements."""
    vals = R.int_values((count, ld), seed)                                    # the columns cols..ld hold values too: never read
    flat = torch.full((src_offset + count * ld,), 5.0, dtype=sdt, device="cuda")
    flat[src_offset:] = vals.reshape(-1).to(sdt)
    dst0 = R.int_values((cols,), seed + 1) if acc else None
    dst = Framed(cols, ddt, dst0)
    item = ops.reduce_item(flat, dst.view, count, cols, ld, scale=scale, accumulate=acc, src_offset=src_offset)
    slab = _is_slab(item.src, item.dst, count, cols, ld)
    path = "slab" if slab else ("tree-vec" if _tree_is_vec(item.src, cols, ld, flat.element_size()) else "tree-scalar")
    assert expect is None or path == expect, f"case meant for {expect} runs {path}"
    ops.reduce_batch([item])
    ref = R.reduce_ref(vals[:, :cols], scale, dst0)
    dst.check(f"reduce {path} count={count} cols={cols} ld={ld}")
    return R.judge_exact(dst.view, ref)


# ---------------------------------------------------------------------------------------------------------------
# colsum / colsum_partial
# ---------------------------------------------------------------------------------------------------------------
COLSUM_N = [1, 3, 4, 5, 15, 16, 17, 19, 127, 128, 129, 128 + 13, 3 * 128 + 1]
COLSUM_C_LD = [(4, 4), (13, 16), (13, 13), (252, 256), (256, 256), (260, 264), (1001, 1001)]


@pytest.mark.parametrize("offset", [0, 1])
@pytest.mark.parametrize("in_dtype", [F32, BF16])
def test_colsum_exact(ops, in_dtype, offset):
    """part row by row against the sums of the 128-row blocks, then kvq_colsum's final sum into f32 and bf16 destinations.  With
    offset 1 the base pointer sits one element past a 16-byte boundary at ld % 4 == 0: every lane must take the scalar path."""
    from kvq._ffi import check, io_dtype_of, lib, stream_ptr
    l = lib()
    combos = itertools.cycle(SCALE_ACC)
    for (C, ld), N in itertools.product(COLSUM_C_LD, COLSUM_N):
        if offset and ld % 4 != 0:
            continue
        vals = R.int_values((N, ld), N * 1009 + C)
        flat = torch.full((offset + N * ld,), 5.0, dtype=in_dtype, device="cuda")
        flat[offset:] = vals.reshape(-1).to(in_dtype)
        x = flat[offset:].view(N, ld)
        assert x.data_ptr() % 16 == offset * flat.element_size()
        P = l.kvq_colsum_partial_rows(N)
        assert P == (N + 127) // 128
        part = Framed(P * C, F32)
        check(l.kvq_colsum_partial(x.data_ptr(), N, C, ld, io_dtype_of(x), part.view.data_ptr(), P * C * 4, stream_ptr()), "colsum_partial")
        what = f"colsum N={N} C={C} ld={ld} {in_dtype} offset={offset}"
        part.check(what)
        ref_part = R.block_sums(vals[:, :C], 128)
        wrong_rows = [p for p in range(P) if R.judge_exact(part.view.view(P, C)[p], ref_part[p])]
        assert not wrong_rows, f"{what}: partial rows {wrong_rows} differ from the exact block sums"
        ws = torch.empty(l.kvq_colsum_workspace_bytes(N, C), dtype=torch.uint8, device="cuda")
        for out_dtype in (F32, BF16):
            scale, acc = next(combos)
            dst0 = R.int_values((C,), N + C) if acc else None
            out = Framed(C, out_dtype, dst0)
            check(l.kvq_colsum(x.data_ptr(), N, C, ld, io_dtype_of(x), out.view.data_ptr(), io_dtype_of(out.view), scale, int(acc),
                               ws.data_ptr(), ws.numel(), stream_ptr()), "colsum")
            out.check(what)
            wrong = R.judge_exact(out.view, R.reduce_ref(vals[:, :C], scale, dst0))
            assert wrong == 0, f"{what} -> {out_dtype} scale={scale} accumulate={acc}: {wrong} of {C} sums are not exact"


# ---------------------------------------------------------------------------------------------------------------
# reduce_batch
# ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("sdt,ddt", [(F32, F32), (F32, BF16), (BF16, F32), (BF16, BF16)])
def test_reduce_slab_exact(ops, sdt, ddt):
    combos = itertools.cycle(SCALE_ACC)
    cases = [(count, cols, cols) for cols in (8, 8184, 8192, 8200, 16384 + 8) for count in (1, 2, 4, 5, 6, 8, 9, 31, 32)]
    cases.append((6, 8200, 8200 + 16))                                        # ld > cols
    for count, cols, ld in cases:
        scale, acc = next(combos)
        wrong = _run_item(ops, count, cols, ld, sdt, ddt, scale, acc, count * 31 + cols, expect="slab")
        assert wrong == 0, f"slab count={count} cols={cols} ld={ld} scale={scale} accumulate={acc}: {wrong} sums are not exact"


@pytest.mark.parametrize("sdt,ddt", [(F32, F32), (F32, BF16), (BF16, F32), (BF16, BF16)])
def test_reduce_tree_vector_exact(ops, sdt, ddt):
    """Not slab-eligible (count > 32, cols % 8 == 4 or ld % 8 == 4) but 4-element aligned: 16 column groups x 64 row phases."""
    combos = itertools.cycle(SCALE_ACC)
    cases = [(count, cols, cols) for cols in (4, 60, 64, 68, 132) for count in (33, 63, 64, 65, 127, 128, 129, 191, 192, 193, 1024)]
    cases += [(count, 64, 68) for count in (33, 129, 1024)]                   # ld % 8 == 4
    cases += [(count, cols, cols) for cols in (4, 68) for count in (1, 5, 32)]   # count <= 32 kept off the slab path by cols % 8 == 4
    cases += [(8, 64, 68)]                                                    # ... and by ld % 8 == 4
    for count, cols, ld in cases:
        scale, acc = next(combos)
        wrong = _run_item(ops, count, cols, ld, sdt, ddt, scale, acc, count * 37 + cols, expect="tree-vec")
        assert wrong == 0, f"tree-vec count={count} cols={cols} ld={ld} scale={scale} accumulate={acc}: {wrong} sums are not exact"


@pytest.mark.parametrize("sdt,ddt", [(F32, F32), (F32, BF16), (BF16, F32), (BF16, BF16)])
def test_reduce_tree_scalar_exact(ops, sdt, ddt):
    """cols % 4 != 0, or a source offset that breaks the 4-element alignment: 64 columns x 16 row phases of scalar loads."""
    combos = itertools.cycle(SCALE_ACC)
    for cols, count in itertools.product((1, 63, 64, 65, 1001), (1, 15, 16, 17, 31, 32, 33, 47, 48, 49, 1000)):
        scale, acc = next(combos)
        off = 1 if cols % 4 == 0 else 0
        wrong = _run_item(ops, count, cols, cols, sdt, ddt, scale, acc, count * 41 + cols, src_offset=off, expect="tree-scalar")
        assert wrong == 0, f"tree-scalar count={count} cols={cols} offset={off} scale={scale} accumulate={acc}: {wrong} sums are not exact"


def _lookup_specs():
    """(path, count, cols, ld, src_offset) of 32 items: a one-block tree item, a 3-block slab item, a one-block and a 2-block slab
    item, then tree items of 2 and 4 .. 30 blocks, alternately scalar and vector: the block counts differ wherever they can."""
    specs = [("tree-scalar", 7, 63, 63, 0), ("slab", 5, 2 * 8192 + 8, 2 * 8192 + 8, 0), ("slab", 32, 8, 8, 0),
             ("tree-vec", 40, 68, 68, 0), ("slab", 3, 8200, 8208, 0)]
    for b in range(4, 31):
        if b % 2:
            specs.append(("tree-scalar", 17 + b, 64 * (b - 1) + 1, 64 * (b - 1) + 1, 0))
        else:
            specs.append(("tree-vec", 60 + b, 64 * (b - 1) + 4, 64 * (b - 1) + 8, 0))
    assert len(specs) == 32
    return specs


def _build_items(ops, specs, seed0):
    dts = itertools.cycle([(F32, F32), (BF16, BF16), (F32, BF16), (BF16, F32)])
    combos = itertools.cycle(SCALE_ACC)
    items, keep = [], []
    for i, (path, count, cols, ld, off) in enumerate(specs):
        sdt, ddt = next(dts)
        scale, acc = next(combos)
        vals = R.int_values((count, ld), seed0 + i)                           # every item its own pattern
        flat = torch.full((off + count * ld,), 5.0, dtype=sdt, device="cuda")
        flat[off:] = vals.reshape(-1).to(sdt)
        dst0 = R.int_values((cols,), seed0 + 1000 + i) if acc else None
        dst = Framed(cols, ddt, dst0)
        it = ops.reduce_item(flat, dst.view, count, cols, ld, scale=scale, accumulate=acc, src_offset=off)
        got = "slab" if _is_slab(it.src, it.dst, count, cols, ld) else \
            ("tree-vec" if _tree_is_vec(it.src, cols, ld, flat.element_size()) else "tree-scalar")
        assert got == path, f"item {i} meant for {path} runs {got}"
        items.append(it)
        keep.append((flat, dst, R.reduce_ref(vals[:, :cols], scale, dst0), f"item {i} ({path} count={count} cols={cols})"))
    return items, keep


def test_reduce_item_lookup_full_launch(ops):
    """One launch of exactly KVQ_REDUCE_MAX_ITEMS items: every workgroup must find its item by the count over first_block[]."""
    from kvq import _ffi
    assert _ffi.KVQ_REDUCE_MAX_ITEMS == 32
    specs = _lookup_specs()
    blocks = [(c + 8191) // 8192 if p == "slab" else (c + 63) // 64 for p, _, c, _, _ in specs]
    assert blocks[:3] == [1, 3, 1] and len(set(blocks)) >= 30
    items, keep = _build_items(ops, specs, 500)
    arr = (_ffi.ReduceItem * 32)(*items)
    _ffi.check(_ffi.lib().kvq_reduce_batch(arr, 32, _ffi.stream_ptr()), "kvq_reduce_batch")
    bad = []
    for flat, dst, ref, what in keep:
        dst.check(what)
        if R.judge_exact(dst.view, ref):
            bad.append(what)
    assert not bad, f"wrong destinations: {bad}"


def test_reduce_37_items_two_launches(ops):
    """More than KVQ_REDUCE_MAX_ITEMS items through nnops.reduce_batch (two launches), every destination checked."""
    specs = _lookup_specs() + [("tree-scalar", 3, 5, 5, 0), ("slab", 4, 16, 16, 0), ("tree-vec", 33, 4, 4, 0),
                               ("tree-scalar", 16, 64, 64, 1), ("slab", 9, 8192, 8192, 0)]
    assert len(specs) == 37
    items, keep = _build_items(ops, specs, 900)
    ops.reduce_batch(items)
    bad = []
    for flat, dst, ref, what in keep:
        dst.check(what)
        if R.judge_exact(dst.view, ref):
            bad.append(what)
    assert not bad, f"wrong destinations: {bad}"


# ---------------------------------------------------------------------------------------------------------------
# sum_slabs
# ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", [F32, BF16])
def test_sum_slabs_exact(ops, dtype):
    for S, n in itertools.product((1, 2, 5), (4, 8, 1020, 256 * 4 * 3 + 4)):
        vals = R.int_values((S, n), S * 100 + n)
        part = vals.to(dtype).cuda()
        out = Framed(n, dtype)
        ops.sum_slabs(part, out.view)
        out.check(f"sum_slabs S={S} n={n}")
        wrong = R.judge_exact(out.view, R.reduce_ref(vals))
        assert wrong == 0, f"sum_slabs S={S} n={n} {dtype}: {wrong} sums are not exact"
