"""The dropout keep mask of the any-length encoder attention entries (include/bayeformers_amd_encoder_any.h), from the
oracle's restatement of the dropout contract: with Tp = 128 * ceil(T / 128) the group of probability (b, h, q, key) is
((((b*H + h)*T + q) * (Tp/32)) + (key // 128)*4 + c) * 4 + lg with key % 128 = (2c + e)*16 + 4 lg + j, field e*4 + j."""
import numpy as np
import torch

from oracle import bayes_oracle as bo


def padded_length(T):
    return 128 * ((T + 127) // 128)


def attention_keep_mask_any(B, H, T, p, seed, call, site, first_group=0, with_pad_keys=False):
    """[B, H, T(query), T(key)] keep mask (uint8, 1 = kept) of bf_attention_fwd_any_dropout; with_pad_keys: [B, H, T, Tp],
    the meaningless decisions of the keys >= T included (the stored keep words carry them)."""
    Tp = padded_length(T)
    keep = bo.dropout_keep(first_group, B * H * T * (Tp // 8), p, seed, call, site)
    keep = keep.reshape(B, H, T, Tp // 128, 4, 4, 8)  # [.., tile, c, lg, field]
    out = np.empty((B, H, T, Tp), dtype=np.uint8)
    for tile in range(Tp // 128):
        for c in range(4):
            for lg in range(4):
                for e in range(2):
                    k0 = tile * 128 + (2 * c + e) * 16 + 4 * lg
                    out[..., k0:k0 + 4] = keep[:, :, :, tile, c, lg, e * 4:e * 4 + 4]
    return out if with_pad_keys else np.ascontiguousarray(out[..., :T])


def keep_words_any(keep_padded):
    """The entries' keep words [.., T, Tp/32] (int32) from a [.., T, Tp] keep mask (torch): word (query, key tile, lg),
    bit c*8 + e*4 + j."""
    Tp = keep_padded.shape[-1]
    km = keep_padded.to(torch.int64).reshape(*keep_padded.shape[:-1], Tp // 128, 8, 4, 4)  # [.., tile, 2c + e, lg, j]
    dev = keep_padded.device
    bit = torch.arange(8, device=dev)[:, None, None] * 4 + torch.arange(4, device=dev)[None, None, :]
    w = (km << bit).sum((-3, -1))  # [.., tile, lg]
    w = torch.where(w >= 2 ** 31, w - 2 ** 32, w).to(torch.int32)
    return w.reshape(*keep_padded.shape[:-1], Tp // 32)
