"""DrM building blocks (DrQV2Agent.dormant_ratio / perturb, drq_dormant_scores / _count, drq_lerp_flat): everything that
needs no GPU.  The numpy restatement of the contract (tests/dormant_oracle.py) on its edge cases, the host helpers of
utils.py, the agent's validation on the CPU, and the argument errors the library reports before any launch."""
import math
import os

import numpy as np
import pytest
import torch

from drqv2_amd import _lib
from tests import abi
from tests import dormant_oracle as DO

NEW = ("drq_dormant_scores", "drq_dormant_count", "drq_lerp_flat")
EARG = -1


def cpu_agent():
    import drqv2
    with torch.random.fork_rng(devices=[]):
        torch.manual_seed(0)
        return drqv2.DrQV2Agent((9, 84, 84), (3,), "cpu", 1e-3, 20, 64, 0.01, 2000, 2, "0.2", 0.3, True)


def test_header_prototypes_and_build_list():
    for name in NEW:
        abi.assert_prototype(name)
        assert hasattr(_lib.load(), name)
    from drqv2_amd import build, ops
    assert "dormant.hip" in build.SOURCES and os.path.exists(os.path.join(build.CSRC, "dormant.hip"))
    assert "fmaf(a, p[i], (1 - a) * p0[i])" in abi.text()            # the expression the oracle restates
    assert all(callable(getattr(ops, n)) for n in ("dormant_scores", "dormant_count", "lerp_flat"))


# ------------------------------------------------------------------------------------------------ the oracle on its own
def test_oracle_zero_layer_is_fully_dormant():
    for units in (1, 50, 1030):
        assert DO.count(np.zeros(units, np.float32), 0.025) == (units, units, 0.0)
        assert DO.count(np.zeros(units, np.float32), 0.0) == (units, units, 0.0)


def test_oracle_one_live_unit_among_zeros():
    for units, live in ((2, 0), (50, 49), (1030, 517)):
        s = np.zeros(units, np.float32)
        s[live] = 3.0
        d, u, m = DO.count(s, 0.025)
        assert (d, u) == (units - 1, units) and m == np.float32(np.float32(3.0) / np.float32(units))
        assert DO.count(s, 0.0)[0] == units - 1
        # tau * m above the live unit's score: tau > units
        assert DO.count(s, 2.0 * units)[0] == units


def test_oracle_scaling_leaves_the_count_unchanged():
    r = np.random.RandomState(0)
    act = r.standard_normal((37, 300)) * (r.uniform(size=300) < 0.7) * r.uniform(0.001, 2.0, 300)
    s = DO.scores(act)
    for tau in (0.025, 0.3, 1.0):
        base = DO.count(s, tau)[0]
        assert 0 < base < 300 or tau == 0.025
        for k in (2.0 ** -20, 0.5, 4.0, 2.0 ** 30):       # powers of two: every operation of the count scales exactly
            assert DO.count(DO.scores(act * k), tau)[0] == base
    assert DO.count(s, 1.0)[0] > DO.count(s, 0.025)[0] >= int((s == 0).sum()) > 50      # the zeroed units at least


def test_oracle_tau_zero_counts_exactly_the_zero_scores():
    r = np.random.RandomState(1)
    s = r.uniform(0.0, 1.0, 777).astype(np.float32)
    s[r.choice(777, 100, replace=False)] = 0.0
    zeros = int((s == 0).sum())
    s[np.flatnonzero(s)[0]] = np.float32(1e-45)                       # the smallest subnormal is not zero
    assert DO.count(s, 0.0)[0] == zeros == 100


def test_oracle_mean_order_and_exact_thresholds():
    s = np.full(1024, 2.0, np.float32)
    s[:256] = 0.5
    assert DO.layer_mean(s) == np.float32(1.625)                      # powers of two: exact in any order
    # scores exactly at the threshold count, one ulp above does not
    for units in (1, 50, 64, 1024, 1030):
        for tau in ((0.25, 1.0) if units == 1 else (0.25,)):
            sc, want = DO.known_scores(units, tau)
            assert DO.count(sc, tau)[:2] == (want, units), (units, tau)
    assert DO.known_scores(1030)[1] == 103 + 5
    # the order matters for general data and is the kernel's: 256 chains, then halves
    r = np.random.RandomState(2)
    x = (r.uniform(0.0, 1.0, 1030) * 10.0 ** r.uniform(-6, 2, 1030)).astype(np.float32)
    chains = np.zeros(256, np.float32)
    for j, v in enumerate(x):
        chains[j % 256] = np.float32(chains[j % 256] + v)
    o = 128
    while o:
        for t in range(o):
            chains[t] = np.float32(chains[t] + chains[t + o])
        o //= 2
    assert DO.layer_mean(x) == np.float32(chains[0] / np.float32(1030))


def test_oracle_lerp_is_the_fused_multiply_add():
    """against exact rational arithmetic, on values built to sit on float32 rounding ties of a * p + q"""
    from fractions import Fraction
    r = np.random.RandomState(3)
    p = (r.standard_normal(4000) * 10.0 ** r.uniform(-3, 3, 4000)).astype(np.float32)
    p0 = (r.standard_normal(4000) * 10.0 ** r.uniform(-3, 3, 4000)).astype(np.float32)
    for a in (0.5, 0.9, 1e-3, 0.999):
        a32 = np.float32(a)
        got = DO.lerp(p, p0, a)
        q = (np.float32(1) - a32) * p0
        for i in range(0, 4000, 7):
            exact = Fraction(float(a32)) * Fraction(float(p[i])) + Fraction(float(q[i]))
            lo = np.float32(float(exact))                              # a candidate; the nearest is it or a neighbour
            cands = (np.nextafter(lo, np.float32(-np.inf)), lo, np.nextafter(lo, np.float32(np.inf)))
            best = min(cands, key=lambda c: (abs(Fraction(float(c)) - exact), int(c.view(np.int32)) & 1))
            assert got[i].tobytes() == best.tobytes(), (a, i)
    assert DO.lerp(p, p0, 1.0).tobytes() == p.tobytes() and DO.lerp(p, p0, 0.0).tobytes() == p0.tobytes()
    # where rounding twice goes wrong: a p = 0.75 + 1.5 * 2^-24 is a float32 tie, q = +-2^-80 far below a float64 ulp
    # of it decides the side; a plain float64 sum drops q and sends both to the even neighbour
    pp = np.array([1.0 + 2.0 ** -23] * 2, np.float32)
    got = DO.lerp(pp, np.array([2.0 ** -78, -2.0 ** -78], np.float32), 0.75)
    assert got[0] == np.float32(0.75 + 2.0 ** -23) and got[1] == np.float32(0.75 + 2.0 ** -24)
    assert np.float32(0.75 * float(pp[0]) + 2.0 ** -80) == np.float32(0.75 * float(pp[0]) - 2.0 ** -80)


def test_perturb_factor_and_dormant_stddev():
    import utils
    assert utils.perturb_factor(0.0, 2.0, 0.2, 0.9) == 0.9            # 1 - 0 = 1 clipped to hi
    assert utils.perturb_factor(0.05, 2.0, 0.2, 0.9) == 0.9           # exactly hi
    assert utils.perturb_factor(0.1, 2.0, 0.2, 0.9) == pytest.approx(0.8)
    assert utils.perturb_factor(0.4, 2.0, 0.2, 0.9) == pytest.approx(0.2)
    assert utils.perturb_factor(1.0, 2.0, 0.2, 0.9) == 0.2            # 1 - 2 = -1 clipped to lo
    assert utils.perturb_factor(torch.tensor(0.25), 2.0, 0.0, 1.0) == 0.5 and isinstance(utils.perturb_factor(0.25, 2, 0, 1), float)
    assert utils.dormant_stddev(0.2, 0, "0.1", target=0.2, temperature=0.1) == 0.5
    assert utils.dormant_stddev(0.0, 0, "linear(1.0,0.1,100)", target=0.2, temperature=0.1) == 1.0
    assert utils.dormant_stddev(0.0, 100, "linear(1.0,0.1,100)", target=0.2, temperature=0.1) == pytest.approx(1 / (1 + math.e ** 2))
    assert utils.dormant_stddev(1.0, 10 ** 6, "0.1", target=0.2, temperature=1e-4) == 1.0
    assert utils.dormant_stddev(0.0, 10 ** 6, "0.1", target=0.2, temperature=1e-4) == 0.1


# ------------------------------------------------------------------------------------------------ the agent on the CPU
def snapshot(ag):
    return (ag._engine.params.clone(), ag._engine.adam_m.clone(), torch.random.get_rng_state(),
            ag.encoder_opt.t, ag.actor_opt.t, ag.critic_opt.t)


def unchanged(ag, snap):
    now = snapshot(ag)
    return all(torch.equal(a, b) if torch.is_tensor(a) else a == b for a, b in zip(snap, now))


def test_cpu_agent_fails_loudly_before_touching_state():
    ag = cpu_agent()
    snap = snapshot(ag)
    obs = torch.zeros((2, 9, 84, 84), dtype=torch.uint8)
    with pytest.raises(_lib.DrqError, match="GPU"):
        ag.dormant_ratio(obs)
    with pytest.raises(_lib.DrqError, match="GPU"):
        ag.dormant_ratio(obs, torch.zeros(2, 3), nets=("actor", "critic"))
    for alpha in (0.0, 0.5, 1.0):
        with pytest.raises(_lib.DrqError, match="GPU"):
            ag.perturb(alpha)
    g = torch.Generator().manual_seed(5)
    gs = g.get_state()
    with pytest.raises(_lib.DrqError, match="GPU"):
        ag.perturb(0.5, generator=g)
    assert torch.equal(g.get_state(), gs) and unchanged(ag, snap) and ag.last_dormant is None


def test_argument_validation():
    ag = cpu_agent()
    snap = snapshot(ag)
    obs = torch.zeros((2, 9, 84, 84), dtype=torch.uint8)
    for alpha in (-0.1, 1.0001, 2, float("nan"), float("inf"), True, False, None, "x", -1e-9):
        with pytest.raises(ValueError, match="alpha"):
            ag.perturb(alpha)
    for tau in (-0.025, -1e-30, float("nan"), float("inf"), True, None, 1e39):
        with pytest.raises(ValueError, match="tau"):
            ag.dormant_ratio(obs, tau=tau)
    for nets in (("policy",), ("actor", "target"), (), ("actor", "actor"), "encoder", (1,), None):
        with pytest.raises(ValueError, match="nets"):
            ag.dormant_ratio(obs, nets=nets)
    for nets in (("target",), ("encoder", "critic_target"), (), ("actor", "actor"), "enc", None):
        with pytest.raises(ValueError, match="nets"):
            ag.perturb(0.5, nets=nets)
    for nets in (("critic",), ("actor", "critic"), "critic"):
        with pytest.raises(ValueError, match="action"):
            ag.dormant_ratio(obs, nets=nets)
    for gen in (5, "g", torch.zeros(3)):
        with pytest.raises(ValueError, match="generator"):
            ag.perturb(0.5, generator=gen)
    assert unchanged(ag, snap)


def test_data_parallel_engine_refuses_perturb():
    ag = cpu_agent()
    ag._engine.device = torch.device("cuda", 0)            # only the refusal is reached
    ag.device = "cuda"
    ag._engine.pg = object()
    snap = snapshot(ag)
    with pytest.raises(_lib.DrqError, match="data parallelism"):
        ag.perturb(0.5)
    with pytest.raises(_lib.DrqError, match="data parallelism"):
        ag._engine.perturb(0.5, {})
    assert unchanged(ag, snap)


# ------------------------------------------------------------------------------------------------ refusals without a GPU
def test_entries_refuse_bad_arguments_before_any_launch():
    """host memory stands in for the device's: a refused call launches nothing, so nothing is ever dereferenced"""
    lib = _lib.load()
    act, score = torch.ones(6, 8), torch.full((8,), 7.0)
    cnt, mean = torch.full((2,), 3, dtype=torch.int32), torch.full((1,), 9.0)
    a, s, c, m = act.data_ptr(), score.data_ptr(), cnt.data_ptr(), mean.data_ptr()
    assert lib.drq_dormant_scores(None, 8, 6, 8, s, None) == EARG and lib.drq_dormant_scores(a, 8, 6, 8, None, None) == EARG
    for ld, rows, units in ((8, 0, 8), (8, -1, 8), (8, 6, 0), (8, 6, -2), (7, 6, 8), (0, 6, 8)):
        assert lib.drq_dormant_scores(a, ld, rows, units, s, None) == EARG, (ld, rows, units)
    assert lib.drq_dormant_count(None, 8, 0.025, c, m, None) == EARG and lib.drq_dormant_count(s, 8, 0.025, None, m, None) == EARG
    for units, tau in ((0, 0.025), (-1, 0.025), (8, -0.025), (8, float("nan")), (8, float("inf")), (8, -0.0 - 1e-30)):
        assert lib.drq_dormant_count(s, units, tau, c, m, None) == EARG, (units, tau)
    p, p0 = torch.full((9,), 1.0), torch.full((9,), 2.0)
    for n, al in ((-1, 0.5), (9, -0.1), (9, 1.5), (9, float("nan")), (9, float("inf"))):
        assert lib.drq_lerp_flat(p.data_ptr(), p0.data_ptr(), n, al, None) == EARG, (n, al)
    assert lib.drq_lerp_flat(None, p0.data_ptr(), 9, 0.5, None) == EARG and lib.drq_lerp_flat(p.data_ptr(), None, 9, 0.5, None) == EARG
    assert lib.drq_lerp_flat(p.data_ptr() + 2, p0.data_ptr(), 4, 0.5, None) == EARG      # not 4-byte aligned
    # the two calls that are complete without a launch
    assert lib.drq_lerp_flat(None, None, 0, 0.5, None) == 0 and lib.drq_lerp_flat(p.data_ptr(), p0.data_ptr(), 9, 1.0, None) == 0
    assert bool((score == 7).all()) and cnt.tolist() == [3, 3] and float(mean) == 9.0
    assert bool((p == 1).all()) and bool((p0 == 2).all())
