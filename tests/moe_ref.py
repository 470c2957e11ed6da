"""A float64 restatement of the Bayesian mixture-of-experts contract (include/bayeformers_amd_moe.h), for the tests: the route
of the slots to their (sample, expert) groups, the gated product, the down product and the combine, on explicit sampled
weights.  Rows are sample-major (row r belongs to sample r // M, M = R // S); a slot is a (row, j) pair numbered r * k + j; its
group is s * E + top_k_index[r, j]; an index equal to E is a dropped slot that contributes nothing.  CPU tensors only."""
import torch

TILE_ROWS = 16


def route(top_k_index, S, E):
    """(offsets [S*E + 1], slots [live]) int64: the live slots sorted by group, in slot order inside a group."""
    R, k = top_k_index.shape
    M = R // S
    idx = top_k_index.reshape(-1).long().cpu()
    slot = torch.arange(R * k)
    live = (idx >= 0) & (idx < E)
    group = (slot // k // M) * E + idx
    group, slot = group[live], slot[live]
    order = torch.sort(group, stable=True).indices
    counts = torch.bincount(group, minlength=S * E)
    offsets = torch.zeros(S * E + 1, dtype=torch.long)
    offsets[1:] = counts.cumsum(0)
    return offsets, slot[order]


def tiles(offsets, max_tiles, rows=TILE_ROWS):
    """[max_tiles, 3] {group, first position, live rows}: every group's tiles in group order, zeros for the surplus."""
    out = torch.zeros((max_tiles, 3), dtype=torch.long)
    t = 0
    for g in range(offsets.numel() - 1):
        lo, hi = int(offsets[g]), int(offsets[g + 1])
        for first in range(lo, hi, rows):
            out[t] = torch.tensor([g, first, min(rows, hi - first)])
            t += 1
    return out


def max_tiles(S, E, R, k, rows=TILE_ROWS):
    return (R * k) // rows + min(S * E, R * k)


def gate_up(x, top_k_index, w_gu, S, act=torch.nn.functional.silu):
    """h [R*k, I] float64: act(gate) * up per slot, gate = features 0 .. I-1 and up = I .. 2I-1 of x w_gu[s, e]^T; rows of
    dropped slots are zero."""
    R, k = top_k_index.shape
    M = R // S
    E, I = w_gu.shape[1], w_gu.shape[2] // 2
    x, w = x.double().cpu(), w_gu.double().cpu()
    h = torch.zeros(R * k, I, dtype=torch.float64)
    for r in range(R):
        for j in range(k):
            e = int(top_k_index[r, j])
            if 0 <= e < E:
                gu = w[r // M, e] @ x[r]
                h[r * k + j] = act(gu[:I]) * gu[I:]
    return h


def down(h, top_k_index, w_d, S):
    """y [R, k, H] float64: y[r, j] = h[r * k + j] w_d[s, e]^T; rows of dropped slots are zero."""
    R, k = top_k_index.shape
    M = R // S
    E, H = w_d.shape[1], w_d.shape[2]
    h, w = h.double().cpu(), w_d.double().cpu()
    y = torch.zeros(R, k, H, dtype=torch.float64)
    for r in range(R):
        for j in range(k):
            e = int(top_k_index[r, j])
            if 0 <= e < E:
                y[r, j] = w[r // M, e] @ h[r * k + j]
    return y


def live_mask(top_k_index, E):
    idx = top_k_index.cpu()
    return (idx >= 0) & (idx < E)


def combine(y, top_k_index, top_k_weights, E):
    """out [R, H] float64: sum_j top_k_weights[r, j] * y[r, j] over the live slots."""
    w = torch.where(live_mask(top_k_index, E), top_k_weights.double().cpu(), torch.zeros((), dtype=torch.float64))
    return (w[:, :, None] * torch.where(live_mask(top_k_index, E)[:, :, None], y.double().cpu(),
                                        torch.zeros((), dtype=torch.float64))).sum(1)


def forward(x, top_k_index, top_k_weights, w_gu, w_d, S, act=torch.nn.functional.silu):
    """The whole layer in float64 on explicit sampled weights w_gu [S, E, 2I, H] and w_d [S, E, H, I]: vectorised (batched
    matmuls per slot's group) and differentiable in x, top_k_weights, w_gu and w_d."""
    R, k = top_k_index.shape
    M = R // S
    E, I = w_gu.shape[1], w_gu.shape[2] // 2
    idx = top_k_index.long()
    live = (idx >= 0) & (idx < E)
    sample = (torch.arange(R, device=idx.device) // M)[:, None].expand(R, k)
    g = sample * E + torch.where(live, idx, torch.zeros_like(idx))
    wg = w_gu.double().reshape(S * E, 2 * I, -1)[g]            # [R, k, 2I, H]
    wd = w_d.double().reshape(S * E, -1, I)[g]                 # [R, k, H, I]
    gu = torch.einsum("rkih,rh->rki", wg, x.double())
    h = act(gu[..., :I]) * gu[..., I:]
    y = torch.einsum("rkhi,rki->rkh", wd, h)
    w = torch.where(live, top_k_weights.double(), torch.zeros((), dtype=torch.float64, device=idx.device))
    return (w[:, :, None] * y).sum(1)


def eps_host(shape, seed, base, S, stream_id):
    """[S, *shape] float64: the generator's epsilon for samples base .. base + S - 1 of one tensor (its host twin)."""
    from bayeformers_amd import ops

    n = 1
    for d in shape:
        n *= d
    return torch.stack([ops.philox_normal_host(n, seed, base + s, stream_id).double().view(*shape) for s in range(S)])


def sample(mu, rho, eps):
    """W_s = mu + softplus(rho) * eps_s in float64."""
    return mu.double()[None] + torch.nn.functional.softplus(rho.double())[None] * eps
