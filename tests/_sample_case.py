"""The tiny engines of tests/test_sample_engine_gpu.py: kvq-bert-tiny (2 layers, 2 heads, H = 128, V = 2048, 64 positions), built as
tests/test_generate_engine_gpu.py builds them -- Shelgon with a VectorQuantizer (K = 32), latents = codebook rows of seeded random
indices; Bagon, seeded normal latents.  B = 6, Se = 12, max_length = 20.  One engine per (kind, dtype), shared by the tests."""
import functools

import torch

K = 32
B, SE, L, H, V = 6, 12, 20, 128, 2048
START = 101                              # [CLS]
SEED = 1


def build(kind):
    from models.bagon.Bagon import Bagon
    from models.shelgon3.Shelgon import Shelgon
    from models.shelgon3.VectorQuantizer import VectorQuantizer
    torch.manual_seed(0)
    if kind == "bagon":
        return Bagon("kvq-bert-tiny", "kvq-bert-tiny", True, compute_dtype=torch.float32)
    vq = VectorQuantizer(K, 128, 0.25, vq_codebook_init_values=torch.randn(K, 128))
    vq.materialize_min_encodings = False
    return Shelgon("kvq-bert-tiny", vq, "kvq-bert-tiny", None, compute_dtype=torch.float32)


def latents_of(kind, model, seed, n=B):
    """f32 latents [n, SE, H] on the CPU and, for Shelgon, the indices they are the codebook rows of"""
    g = torch.Generator().manual_seed(seed)
    if kind == "bagon":
        return torch.randn((n, SE, H), generator=g), None
    idx = torch.randint(0, K, (n, SE), generator=g)
    return model.vector_quantizer.embedding.weight.detach().float().cpu()[idx], idx


@functools.lru_cache(maxsize=None)
def case(kind, dtype):
    from kvq.engine import engine_of
    model = build(kind)
    lat32, idx = latents_of(kind, model, SEED)
    model.compute_dtype = dtype
    model = model.cuda().eval()
    eng = engine_of(model)
    assert eng.dtype == dtype and eng.V == V
    lat = lat32.to(dtype).cuda().contiguous()
    prompt = torch.full((B, 1), START, dtype=torch.int64, device="cuda")
    with torch.no_grad():
        greedy = eng.generate(lat, L, prompt)
    torch.cuda.synchronize()
    return dict(model=model, eng=eng, lat=lat, idx=None if idx is None else idx.cuda(), prompt=prompt, greedy=greedy)
