"""SHA-256 digests of what the twelve decoder-block wrappers of `ops` return, on the device.

    python tests/golden/make_decoder_block_digests.py            # rewrites tests/golden/decoder_block_digests.json
    python tests/golden/make_decoder_block_digests.py --list     # every call's digests, one per line (to diff two builds)

The kernels behind add_rmsnorm / rope_qk / swiglu, norm_add_rmsnorm / qknorm_rope / geglu and their six backwards promise
the same bits from one build to the next: no atomics, every reduction in a fixed order.  The file records those bits at the
commit that last meant to change them; tests/test_gpu_decoder_block_digests.py replays the grid against it, so a refactor
of the kernels, their launchers or the wrappers must reproduce it unchanged.  It is only ever regenerated on purpose.

Inputs are drawn on the CPU from seeded torch.Generators in fp32, cast to the case's dtype and moved to the device.  A
group is (op, activation dtype, dtype of the gammas or tables, weight offset); its digest is the SHA-256 over, for every
call of the group in order, the call's name and the SHA-256 of each output's raw bytes.  The JSON holds one digest per
group: names and digests only.

The grid
  dtypes   bf16, fp16, fp32; gammas (and the rotary tables) fp32 or of the activation dtype; weight offset 0 and 1
  gammas   entry 1 is -0.0 and entry 2 is 0.0 (a (0 + gamma) that loses the sign of -0.0 flips the sign of a zero output)
  norms    N 8 (a lone vector), 256 / 768 / 1024 (half a wave per row, 1 / 3 / 4 vectors), 1032 (a wave per row, idle
           vectors), 2056 and 4104 (forward 8 and 16 vectors; backward the workgroup on a row, 2 and 4), 8192 (the limit);
           rows 1, 5 (an idle half-wave, an idle group in the last round), 9 (a second workgroup); with and without the
           residual, gamma_pre, the sum output, dz_in, and dy = None for the family entry; backward also (rows 8195, N 256)
           and (rows 520, N 2056), past the workgroup caps: the row loop and the fixed-order sum of the partials run twice
  rotary   B 2, T 3, H 4, Hkv 2, tables for one batch and for B, q / k transposed views of [B, T, heads * D], in place and
           out of place; D 64 / 128 for rope_qk, and 256 and the gammas (both, q's, k's, none) for qknorm_rope, whose tables for
           B batches have the dtype the gammas have not (fp32 against the activations'); the backward
           reads gradients laid out [B, heads, T, D]; one bf16 case B 1, T 4096, H 32, Hkv 8, D 128 past both grid caps
  gates    N 8 / 64 / 2056, rows 1 / 5 and (rows 8200, N 64) for the row loop; contiguous tensors and the two halves of a
           stacked [rows, 2 N] buffer, stacked=True in the backward; the first gates of every tensor are +-0, +-88.8, +-100
           and +-1e5 (+-6e4 in fp16, whose largest finite value is 65504)
"""
import hashlib
import json
import os
import sys
import zlib

import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))  # the repository root, when run as a script

from bayeformers_amd import ops  # noqa: E402

JSON_PATH = os.path.join(HERE, "decoder_block_digests.json")

DTYPES = {"bf16": torch.bfloat16, "fp16": torch.float16, "fp32": torch.float32}
NORM_N = (8, 256, 768, 1024, 1032, 2056, 4104, 8192)
NORM_ROWS = (1, 5, 9)
NORM_BIG = ((8195, 256), (520, 2056))
ROPE_SHAPE = dict(B=2, T=3, H=4, Hkv=2)
ROPE_BIG = dict(B=1, T=4096, H=32, Hkv=8)
GLU_SHAPES = tuple((rows, n) for n in (8, 64, 2056) for rows in (1, 5)) + ((8200, 64),)
EPS_PRE, EPS_OUT = 1e-6, 1e-5

_CPU = {}


def _draw(tag, shape, scale=1.0):
    """fp32 CPU normal draws for (tag, shape): the same tensor every time it is asked for."""
    key = (tag, tuple(shape), scale)
    if key not in _CPU:
        gen = torch.Generator().manual_seed(zlib.crc32(repr(key).encode()))
        _CPU[key] = torch.randn(*shape, generator=gen) * scale
    return _CPU[key]


def _dev(tag, shape, dtype, scale=1.0):
    return _draw(tag, shape, scale).to(dtype).to("cuda")


def _gamma(tag, n, dtype):
    g = _draw(tag, (n,), 0.3).clone()
    g[1], g[2] = -0.0, 0.0
    return g.to(dtype).to("cuda")


def _sha(t):
    return hashlib.sha256(t.detach().contiguous().cpu().view(torch.uint8).numpy().tobytes()).hexdigest()


def groups():
    """[(group name, function yielding (call name, [output tensors or None]))], in the JSON's order."""
    out = []
    for dn, dt in DTYPES.items():
        for gn, gdt in ((("fp32", torch.float32),) if dn == "fp32" else (("fp32", torch.float32), (dn, dt))):
            out.append((f"add_rmsnorm|{dn}|{gn}", lambda dt=dt, gdt=gdt: _add_rmsnorm(dt, gdt)))
            out.append((f"add_rmsnorm_backward|{dn}|{gn}", lambda dt=dt, gdt=gdt: _add_rmsnorm_bwd(dt, gdt)))
            out.append((f"rope_qk|{dn}|{gn}", lambda dt=dt, gdt=gdt: _rope(dt, gdt, False)))
            out.append((f"rope_qk_backward|{dn}|{gn}", lambda dt=dt, gdt=gdt: _rope(dt, gdt, True)))
            for woff in (0, 1):
                out.append((f"norm_add_rmsnorm|{dn}|{gn}|{woff}", lambda dt=dt, gdt=gdt, w=woff: _norm_add(dt, gdt, w)))
                out.append((f"norm_add_rmsnorm_backward|{dn}|{gn}|{woff}",
                            lambda dt=dt, gdt=gdt, w=woff: _norm_add_bwd(dt, gdt, w)))
                out.append((f"qknorm_rope|{dn}|{gn}|{woff}", lambda dt=dt, gdt=gdt, w=woff: _qkrope(dt, gdt, w, False)))
                out.append((f"qknorm_rope_backward|{dn}|{gn}|{woff}",
                            lambda dt=dt, gdt=gdt, w=woff: _qkrope(dt, gdt, w, True)))
        for op in ("swiglu", "geglu"):
            out.append((f"{op}|{dn}", lambda dt=dt, op=op: _glu(dt, op, False)))
            out.append((f"{op}_backward|{dn}", lambda dt=dt, op=op: _glu(dt, op, True)))
    out.append(("rope_big|bf16|fp32", _rope_big))
    return out


# ---- the norms
def _add_rmsnorm(dt, gdt):
    for n in NORM_N:
        g = _gamma("g_out", n, gdt)
        for rows in NORM_ROWS:
            x, r = _dev("x", (rows, n), dt), _dev("res", (rows, n), dt, 3.0)
            for res in (None, r):
                for want_sum in (True, False):
                    z, y = ops.add_rmsnorm(x, res, g, EPS_OUT, want_sum=want_sum)
                    yield f"N{n} rows{rows} res{int(res is not None)} sum{int(want_sum)}", [None if z is x else z, y]


def _norm_add(dt, gdt, woff):
    for n in NORM_N:
        gp, go = _gamma("g_pre", n, gdt), _gamma("g_out", n, gdt)
        for rows in NORM_ROWS:
            x, r = _dev("x", (rows, n), dt), _dev("res", (rows, n), dt, 3.0)
            for pre in (None, gp):
                for res in (None, r):
                    for want_sum in (True, False):
                        z, y = ops.norm_add_rmsnorm(x, pre, res, go, EPS_PRE, EPS_OUT, woff, want_sum=want_sum)
                        yield (f"N{n} rows{rows} pre{int(pre is not None)} res{int(res is not None)} sum{int(want_sum)}",
                               [None if z is x else z, y])


def _norm_shapes():
    return [(rows, n) for n in NORM_N for rows in NORM_ROWS] + list(NORM_BIG)


def _add_rmsnorm_bwd(dt, gdt):
    for rows, n in _norm_shapes():
        g = _gamma("g_out", n, gdt)
        z, dy, dz_in = _dev("z", (rows, n), dt, 3.0), _dev("dy", (rows, n), dt), _dev("dz_in", (rows, n), dt, 0.5)
        for h in (None, dz_in):
            yield f"N{n} rows{rows} dz_in{int(h is not None)}", list(ops.add_rmsnorm_backward(z, g, dy, EPS_OUT, grad_sum=h))


def _norm_add_bwd(dt, gdt, woff):
    for rows, n in _norm_shapes():
        gp, go = _gamma("g_pre", n, gdt), _gamma("g_out", n, gdt)
        x, z = _dev("x", (rows, n), dt), _dev("z", (rows, n), dt, 3.0)
        dy, dz_in = _dev("dy", (rows, n), dt), _dev("dz_in", (rows, n), dt, 0.5)
        for pre in (None, gp):
            for g, h in ((dy, None), (dy, dz_in), (None, dz_in)):
                for want_dz in ((True, False) if pre is not None else (True,)):
                    outs = ops.norm_add_rmsnorm_backward(x if pre is not None else None, z, pre, go, g, EPS_PRE, EPS_OUT, woff,
                                                         grad_sum=h, want_dz=want_dz)
                    dx, dz, dg_pre, dg_out = outs
                    yield (f"N{n} rows{rows} pre{int(pre is not None)} dy{int(g is not None)} dz_in{int(h is not None)} "
                           f"dz{int(want_dz)}", [None if dx is dz else dx, dz, dg_pre, dg_out])


# ---- the rotary embedding
def _qk(tag, dt, B, T, H, Hkv, D):
    """q / k as the projections leave them: [B, heads, T, D] views of fresh [B, T, heads * D] buffers."""
    q = _dev(tag + "q", (B, T, H * D), dt).clone().view(B, T, H, D).transpose(1, 2)
    k = _dev(tag + "k", (B, T, Hkv * D), dt).clone().view(B, T, Hkv, D).transpose(1, 2)
    return q, k


def _tables(cb, T, D, cdt):
    return _dev("cos", (cb, T, D), cdt), _dev("sin", (cb, T, D), cdt)


def _rope(dt, cdt, bwd):
    B, T, H, Hkv = (ROPE_SHAPE[k] for k in ("B", "T", "H", "Hkv"))
    for D in (64, 128):
        for cb in (1, B):
            cos, sin = _tables(cb, T, D, cdt)
            if bwd:
                gq, gk = _dev("gq", (B, H, T, D), dt), _dev("gk", (B, Hkv, T, D), dt)
                yield f"D{D} cos{cb}", list(ops.rope_qk_backward(gq, gk, cos, sin))
                q, k = _qk("g", dt, B, T, H, Hkv, D)  # gradients that arrive as transposed views
                yield f"D{D} cos{cb} views", list(ops.rope_qk_backward(q, k, cos, sin))
            else:
                for inplace in (False, True):
                    q, k = _qk("", dt, B, T, H, Hkv, D)
                    yield f"D{D} cos{cb} inplace{int(inplace)}", list(ops.rope_qk(q, k, cos, sin, inplace=inplace))


def _qkrope(dt, gdt, woff, bwd):
    B, T, H, Hkv = (ROPE_SHAPE[k] for k in ("B", "T", "H", "Hkv"))
    for D in (64, 128, 256):
        g_q, g_k = _gamma("g_q", D, gdt) + 1.0 - woff, _gamma("g_k", D, gdt) + 1.0 - woff
        g_q[1], g_q[2], g_k[1], g_k[2] = -0.0, 0.0, -0.0, 0.0
        for cb in (1, B):
            # the batched tables take the other dtype of the two, so that tables and gammas of unlike dtypes are replayed too
            cos, sin = _tables(cb, T, D, gdt if cb == 1 else (dt if gdt == torch.float32 else torch.float32))
            for which, (a, b) in (("both", (g_q, g_k)), ("q", (g_q, None)), ("k", (None, g_k)), ("none", (None, None))):
                if bwd:
                    gq, gk = _dev("gq", (B, H, T, D), dt), _dev("gk", (B, Hkv, T, D), dt)
                    q, k = _qk("", dt, B, T, H, Hkv, D)
                    yield (f"D{D} cos{cb} gammas-{which}",
                           list(ops.qknorm_rope_backward(gq, gk, cos, sin, q, k, a, b, EPS_PRE, woff)))
                else:
                    for inplace in (False, True):
                        q, k = _qk("", dt, B, T, H, Hkv, D)
                        yield (f"D{D} cos{cb} gammas-{which} inplace{int(inplace)}",
                               list(ops.qknorm_rope(q, k, cos, sin, a, b, eps=EPS_PRE, weight_offset=woff, inplace=inplace)))


def _rope_big():
    dt, D = torch.bfloat16, 128
    B, T, H, Hkv = (ROPE_BIG[k] for k in ("B", "T", "H", "Hkv"))
    cos, sin = _tables(1, T, D, torch.float32)
    g_q, g_k = _gamma("g_q", D, torch.float32) + 1.0, _gamma("g_k", D, torch.float32) + 1.0
    q, k = _qk("big", dt, B, T, H, Hkv, D)
    yield "rope_qk", list(ops.rope_qk(q, k, cos, sin))
    yield "rope_qk_backward", list(ops.rope_qk_backward(q, k, cos, sin))
    yield "qknorm_rope", list(ops.qknorm_rope(q, k, cos, sin, g_q, g_k, eps=EPS_PRE))
    yield "qknorm_rope none", list(ops.qknorm_rope(q, k, cos, sin))
    gq, gk = q.contiguous(), k.contiguous()
    yield "qknorm_rope_backward", list(ops.qknorm_rope_backward(gq, gk, cos, sin, q, k, g_q, g_k, EPS_PRE, 0))
    yield "qknorm_rope_backward none", list(ops.qknorm_rope_backward(gq, gk, cos, sin))


# ---- the gated activations
def _gates(tag, shape, dt):
    g = _draw(tag, shape, 4.0).clone()
    top = 6e4 if dt == torch.float16 else 1e5
    special = torch.tensor([0.0, -0.0, 88.8, -88.8, 100.0, -100.0, top, -top])
    g.view(-1)[:8] = special
    return g.to(dt).to("cuda")


def _glu(dt, op, bwd):
    fwd, back = getattr(ops, op), getattr(ops, op + "_backward")
    for rows, n in GLU_SHAPES:
        gate, up, dy = _gates("gate", (rows, n), dt), _dev("up", (rows, n), dt), _dev("dy", (rows, n), dt)
        both = torch.cat((gate, up), -1)  # a stacked projection's [rows, 2 N] output
        for name, (a, b) in (("contiguous", (gate, up)), ("halves", (both[:, :n], both[:, n:]))):
            if bwd:
                for stacked in (False, True):
                    yield f"N{n} rows{rows} {name} stacked{int(stacked)}", list(back(a, b, dy, stacked=stacked))
            else:
                yield f"N{n} rows{rows} {name}", [fwd(a, b)]


def digest(calls, listing=None):
    """The group's digest; listing: a list that receives one line per call."""
    h = hashlib.sha256()
    for name, outs in calls:
        shas = ["-" if t is None else _sha(t) for t in outs]
        h.update((name + ":" + ",".join(shas) + ";").encode())
        if listing is not None:
            listing.append(name + " " + " ".join(s[:16] for s in shas))
    return h.hexdigest()


def main(argv):
    if not torch.cuda.is_available():
        raise SystemExit("make_decoder_block_digests: no ROCm device; the digests are those of the device's results")
    listing = [] if "--list" in argv else None
    table = {}
    for name, fn in groups():
        mark = len(listing) if listing is not None else 0
        table[name] = digest(fn(), listing)
        if listing is not None:
            for line in listing[mark:]:
                print(name, line)
    if listing is None:
        with open(JSON_PATH, "w") as f:
            f.write("{\n" + ",\n".join(f" {json.dumps(k)}: {json.dumps(v)}" for k, v in table.items()) + "\n}\n")
        print(f"{len(table)} groups, {os.path.getsize(JSON_PATH)} bytes -> {JSON_PATH}")


if __name__ == "__main__":
    sys.exit(main(sys.argv[1:]))
