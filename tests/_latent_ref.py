"""torch float64 restatements of the latent kernels (csrc/kvq_latent.hip), device-agnostic: the checkers of
tests/test_latent_kernels_gpu.py and tests/test_latent_engine_gpu.py; tests/test_latent_host.py checks them against plain torch."""
import torch


def group_sum_ref(x, group, n_groups):
    """(table f64 [G, S, H], count int64 [G], abs f64 [G, S, H] = sum of |x| per cell, n_bad) of x [B, S, H], group [B] int.
    Labels -1 are skipped; labels outside [-1, G) are skipped and counted."""
    B, S, H = x.shape
    xd = x.to(torch.float64)
    table = torch.zeros((n_groups, S, H), dtype=torch.float64, device=x.device)
    mag = torch.zeros_like(table)
    count = torch.zeros(n_groups, dtype=torch.int64, device=x.device)
    n_bad = 0
    for b, g in enumerate(group.tolist()):
        if g == -1:
            continue
        if g < -1 or g >= n_groups:
            n_bad += 1
            continue
        table[g] += xd[b]
        mag[g] += xd[b].abs()
        count[g] += 1
    return table, count, mag, n_bad


def shift_ref(x, table, count, g1, g0, alpha=1.0, sel=None):
    """x + alpha * (table[g1] / count[g1] - table[g0] / count[g0]) where sel != 0 (None: everywhere), x elsewhere: every operation
    in f64, the result rounded to f32 and then to the dtype of x.  A zero count means no shift."""
    if int(count[g1]) == 0 or int(count[g0]) == 0:
        return x.clone()
    d = table[g1] / count[g1].to(torch.float64) - table[g0] / count[g0].to(torch.float64)
    r = (x.to(torch.float64) + float(alpha) * d.unsqueeze(0)).to(torch.float32).to(x.dtype)
    if sel is None:
        return r
    return torch.where((sel != 0).unsqueeze(-1), r, x)


def lookup_ref(codebook, indices, n_codes, dtype):
    """out [N, G * Dg] = the rows codebook[g * K + indices[n, g]] side by side, cast to dtype (codebook f32 [G * K, Dg])."""
    N, G = indices.shape
    rows = codebook[(indices + torch.arange(G, device=indices.device) * n_codes).reshape(-1)]        # [N * G, Dg]
    return rows.reshape(N, G * codebook.shape[1]).to(dtype)


def mean_direction_ref(latents, group, g1, g0):
    """mean over the sentences of group g1 minus the mean over those of g0, f64 [S, H]"""
    xd, group = latents.to(torch.float64), torch.as_tensor(group, device=latents.device)
    return xd[group == g1].mean(0) - xd[group == g0].mean(0)
