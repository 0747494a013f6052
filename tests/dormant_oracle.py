"""The contract of drq_dormant_scores / drq_dormant_count / drq_lerp_flat and of DrQV2Agent.dormant_ratio()
(include/drqv2_hip.h, "dormant ratio and perturbation") stated once more, in numpy and on the oracle's modules:

  scores(act)           float64 mean of |act| over the rows, rounded to float32: what the kernel is held to within the
                        bound of its summation (score_bound), not bit for bit
  layer_mean / count    exact, given float32 scores: the mean in the kernel's own order (256 chains, then halved), the
                        threshold tau * m as one float32 product, `<=`, and "m == 0: every unit".  Compared for equality.
  lerp(p, p0, a)        bit-exact: float32(a * p + float32((1 - a) * p0)), the fused multiply-add emulated in float64.
                        a * p is exact in float64; its sum with the rounded product is rounded to ODD there (TwoSum gives the
                        rounding error) so that the final rounding to float32 is the single rounding of the fma -- a
                        plain float64 sum would round twice and miss by one ulp about once in 2^29 elements.
  forward_layers(...)   the scored layers of the actor and the critic from oracle/drq_oracle.py's functional modules.
A helper module: not collected."""
import numpy as np
import torch

U = 2.0 ** -24
CHAINS = 256


def scores(act):
    return np.abs(np.asarray(act, dtype=np.float64)).mean(axis=0).astype(np.float32)


def score_bound(rows, ref):
    """|kernel - scores()| per unit: a sum of `rows` non-negative terms in any order errs by at most rows * 2^-24
    relative to it; the division, the oracle's own rounding and |.| (exact) add two more roundings."""
    return (rows + 2) * U * np.asarray(ref, dtype=np.float64)


def layer_mean(score):
    s = np.asarray(score, dtype=np.float32)
    c = np.zeros(CHAINS, np.float32)
    for k in range(0, len(s), CHAINS):          # chain t adds s[t], s[t + 256], ... in that order
        chunk = s[k:k + CHAINS]
        c[:len(chunk)] = c[:len(chunk)] + chunk
    o = CHAINS // 2
    while o:                                    # chain t takes chain t + o
        c[:o] = c[:o] + c[o:2 * o]
        o //= 2
    return np.float32(c[0] / np.float32(len(s)))


def count(score, tau):
    """-> (dormant units, units, layer mean)"""
    s = np.asarray(score, dtype=np.float32)
    m = layer_mean(s)
    if m == 0:
        return len(s), len(s), m
    thr = np.float32(np.float32(tau) * m)
    return int((s <= thr).sum()), len(s), m


def known_scores(units, tau=0.25, seed=0):
    """-> (float32 scores, the number of dormant units, by construction).  From 50 units on: a bulk of 1, 2 and 4 (powers
    of two: every partial sum is exact, so the mean is the correctly rounded sum / units in any order), a tenth exact
    zeros, three scores exactly AT tau * m (dormant: `<=`), two one ulp below (dormant) and three one ulp above (not).
    Moving a special score moves m, so the specials are set from the threshold until nothing changes; the assertions
    say that the construction holds for the scores returned.  Fewer units: a single 2.0, dormant exactly when tau >= 1."""
    if units < 50:
        s = np.full(units, 2.0, np.float32)
        return s, (units if tau >= 1.0 else 0)
    r = np.random.RandomState(seed + units)
    s = np.float32(2.0) ** r.randint(0, 3, units).astype(np.float32)
    idx = r.permutation(units)
    nz = units // 10
    zero, at, below, above = idx[:nz], idx[nz:nz + 3], idx[nz + 3:nz + 5], idx[nz + 5:nz + 8]
    s[zero] = 0.0
    up, down = np.float32(np.inf), np.float32(0.0)
    for _ in range(20):
        thr = np.float32(np.float32(tau) * layer_mean(s))
        new = s.copy()
        new[at], new[below], new[above] = thr, np.nextafter(thr, down), np.nextafter(thr, up)
        if new.tobytes() == s.tobytes():
            break
        s = new
    thr = np.float32(np.float32(tau) * layer_mean(s))
    assert 0 < thr < 1 and (s[at] == thr).all() and (s[below] == np.nextafter(thr, down)).all()
    assert (s[above] == np.nextafter(thr, up)).all() and (s[zero] == 0).all()
    return s, nz + 5


def lerp(p, p0, a):
    p, p0 = np.asarray(p, dtype=np.float32), np.asarray(p0, dtype=np.float32)
    a = np.float32(a)
    assert 0 <= a <= 1
    if a == 1:
        return p.copy()                         # the entry launches nothing
    q = (np.float32(1) - a) * p0                # float32 x float32 -> float32, correctly rounded
    assert q.dtype == np.float32
    if a == 0:
        return q                                # (1 - 0) * p0 = p0; p is not read into the result
    x, y = np.float64(a) * p.astype(np.float64), q.astype(np.float64)
    with np.errstate(invalid="ignore"):         # an infinite p: s is infinite and stays
        s = x + y
        bb = s - x
        e = (x - (s - bb)) + (y - bb)           # TwoSum: x + y = s + e exactly
    odd = (s.view(np.int64) & 1) == 1
    fix = (e != 0) & ~odd & np.isfinite(s) & np.isfinite(e)
    s = np.where(fix, np.nextafter(s, np.where(e > 0, np.inf, -np.inf)), s)
    return s.astype(np.float32)


def forward_layers(enc, actor, critic, obs_u8, action=None, nets=("actor",), dtype=torch.float64):
    """{layer name: post-activation output [n, units]} for the layers DrQV2Agent.dormant_ratio scores, in its order.
    enc / actor / critic: state dicts (any float dtype); obs_u8 [n,9,84,84]; action [n,A] for the critic."""
    from oracle import drq_oracle as O
    cast = lambda sd: {k: v.detach().cpu().to(dtype) for k, v in sd.items()}
    feat = O.encoder_forward(cast(enc), obs_u8.cpu().to(dtype))
    out = {}
    for net in nets:
        p = cast(actor if net == "actor" else critic)
        h = O.trunk_forward(p, feat)
        out[f"{net}.trunk"] = h
        if net == "actor":
            heads = (("policy", h),)
        else:
            ha = torch.cat([h, action.cpu().to(dtype)], dim=-1)
            heads = (("Q1", ha), ("Q2", ha))
        for prefix, x in heads:
            rec = []
            O.mlp3(p, prefix, x, rec=rec)
            out[f"{net}.{prefix}.0"] = torch.relu(rec[0][0])
            out[f"{net}.{prefix}.2"] = torch.relu(rec[1][0])
    return out


def ratio_of(layers, tau):
    """(ratio, {layer: (dormant, units, mean, float32 scores)}) of forward_layers()' result"""
    per, nd, nu = {}, 0, 0
    for name, act in layers.items():
        s = scores(act.numpy())
        d, u, m = count(s, tau)
        per[name] = (d, u, m, s)
        nd, nu = nd + d, nu + u
    return nd / nu, per
