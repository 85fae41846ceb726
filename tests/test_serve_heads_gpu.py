"""heads_sample_kernel and gather_obs_kernel (runtime/csrc/
runtime_kernels.hip) through their test bindings, _tbruntime.heads_sample and
_tbruntime.gather_obs, against the oracle of tests/helpers/heads_oracle.py.

Heads, numbers. Logits and baseline of both core forms ([x, reward] and x
alone) per element against float64: bit for bit on the small-integer cases,
within K * 2^-24 * S on the random ones, at every D, A and b of the oracle's
tables, with a sentinel kept in the rows past b. K = 4 r is derived, not
chosen: r = 3.92 is what a plain float32 F.linear on the CPU measures against
float64 over the same cases (tests/test_heads_oracle.py prints it); the
kernel itself measures at most 1.99, at D = 64 with the reward (printed by
the run).

Heads, the draw. The action is a Gumbel-argmax sample from softmax of the
logits the same launch returns. Chi-square per logit vector within one launch
of 200,000 rows and pooled over 500 launches seeded as the runner seeds them
(chi-square limit 56.49 at 1 - 1e-6 of chi2(15); measured on the MI355X:
at most 35.7 within one launch, 26.1 pooled), no draw of an action at logit
-40, agreement of neighbouring rows and of consecutive launches within 5
sigma, determinism, and greedy mode against first-index argmax with exact
ties. The statistics are shown to pass a correct sampler and to reject broken
ones in tests/test_heads_oracle.py.

gather_obs against a numpy gather, bit for bit, and one case per host check
of either binding: each raises before anything is launched.
"""

import os
import sys

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

if not torch.cuda.is_available():  # pragma: no cover
    pytest.skip("requires ROCm GPU", allow_module_level=True)

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)),
                                "helpers"))

import heads_oracle as ho  # noqa: E402
from torchbeast_amd import runtime  # noqa: E402

tb = runtime._tbruntime

CPU_RATIO = 3.92  # measured: float32 F.linear on the CPU vs float64
K = 4 * CPU_RATIO
SENTINEL = -7.0
FORMS = [pytest.param(True, id="x_rew"), pytest.param(False, id="x_only")]


def _outputs(rows, A):
    """Pinned outputs holding the sentinel."""
    return (torch.full((rows,), int(SENTINEL), dtype=torch.int64).pin_memory(),
            torch.full((rows, A), SENTINEL).pin_memory(),
            torch.full((rows,), SENTINEL).pin_memory())


def _gpu(case):
    return {k: (None if v is None else v.cuda()) for k, v in case.items()}


def _heads(g, b, greedy=True, seed=0, rows=None, A=None):
    """One launch on the GPU operands `g`; (action, logits, baseline) with
    `rows` >= b rows each."""
    A = g["policy_w"].shape[0] if A is None else A
    out = _outputs(b + 20 if rows is None else rows, A)
    tb.heads_sample(g["x"], g["rew"], g["policy_w"], g["policy_b"],
                    g["base_w"], g["base_b"], b, greedy, seed, *out)
    return out


def _assert_pad_rows_kept(out, b):
    action, logits, baseline = out
    assert action.shape[0] > b
    assert (action[b:] == int(SENTINEL)).all()
    assert (logits[b:] == SENTINEL).all()
    assert (baseline[b:] == SENTINEL).all()


# ---- numbers ----


def test_k_is_the_oracles():
    assert CPU_RATIO == ho.CPU_RATIO and K == ho.K


@pytest.mark.parametrize("with_rew", FORMS)
@pytest.mark.parametrize("D", ho.D_VALUES)
@pytest.mark.parametrize("kind", ["exact", "bounded"])
def test_heads_match_float64(kind, D, with_rew):
    worst = 0.0
    for A in ho.A_VALUES:
        case = ho.case(kind, D, A, with_rew)
        (ref_l, ref_b), (s_l, s_b) = ho.reference(case)
        g = _gpu(case)
        for b in ho.B_VALUES:
            out = _heads(g, b)
            action, logits, baseline = out
            bad, ratio = ho.judge(
                kind, logits[:b], baseline[:b], (ref_l[:b], ref_b[:b]),
                (s_l[:b], s_b[:b]), K)
            worst = max(worst, ratio)
            assert not bad, f"{kind} D={D} A={A} b={b}: " + "; ".join(bad)
            _assert_pad_rows_kept(out, b)
            assert torch.equal(
                action[:b], torch.from_numpy(np.argmax(logits[:b].numpy(), 1)))
    if kind == "bounded":
        print(f"heads D={D} {'x_rew' if with_rew else 'x_only'}: largest"
              f" ratio {worst:.3f} of 2^-24*S, K = {K:.2f}")


# ---- greedy ----


def _with_ties(case):
    """The exact case's heads with actions made exact copies of others: a
    pair and a triple whose logits tie in every row."""
    c = dict(case)
    pw, pb = case["policy_w"].clone(), case["policy_b"].clone()
    for src, dst in ((10, 7), (4, 5), (4, 11)):
        pw[dst], pb[dst] = pw[src], pb[src]
    c["policy_w"], c["policy_b"] = pw, pb
    return c


@pytest.mark.parametrize("with_rew", FORMS)
def test_greedy_is_first_index_argmax_of_returned_logits(with_rew):
    b = ho.ROWS
    case = _with_ties(ho.exact_case(65, 18, with_rew))
    action, logits, _ = _heads(_gpu(case), b)
    z = logits[:b].numpy()
    top = z == z.max(1, keepdims=True)
    two = int((top[:, 7] & top[:, 10] & (top.sum(1) == 2)).sum())
    three = int((top[:, 4] & top[:, 5] & top[:, 11]
                 & (top.sum(1) == 3)).sum())
    print(f"rows with a two-way tie at the maximum: {two}, three-way: {three}")
    assert two >= 5 and three >= 5
    assert int((top.sum(1) == 1).sum()) >= 50
    want = np.argmax(z, 1)  # first occurrence
    assert np.array_equal(action[:b].numpy(), want)
    # The tied rows answer the first of the copies, never a later one.
    tied3 = top[:, 4] & top[:, 5] & top[:, 11] & (top.sum(1) == 3)
    assert (action[:b].numpy()[tied3] == 4).all()

    # One action: always it, greedy or drawn.
    one = _gpu(ho.exact_case(65, 1, with_rew))
    for greedy in (True, False):
        out = _heads(one, b, greedy=greedy, seed=3)
        assert (out[0][:b] == 0).all()
        _assert_pad_rows_kept(out, b)


# ---- the draw ----


def _vector_heads(A_vectors):
    """Heads whose logits are exactly one of four given vectors, selected by
    a one-hot core: logits[r] = z[r % 4] (a sum of one product by 1 and
    zeros, so exact), baseline 0."""
    z = A_vectors
    A = z.shape[1]
    return dict(policy_w=z.t().contiguous().cuda(),
                policy_b=torch.zeros(A).cuda(),
                base_w=torch.zeros(1, 4).cuda(), base_b=torch.zeros(1).cuda(),
                rew=None)


def _one_hot_rows(rows):
    x = torch.zeros(rows, 4)
    x[torch.arange(rows), torch.arange(rows) % 4] = 1
    return x.cuda()


def test_draw_distribution_within_one_launch():
    z = ho.four_logit_vectors()
    limit = ho.chi2_limit()
    n = ho.N_DRAWS
    g = dict(_vector_heads(z), x=_one_hot_rows(n))
    action, logits, baseline = _heads(g, n, greedy=False, seed=12345, rows=n)
    assert torch.equal(logits, z.repeat(n // 4, 1))
    assert (baseline == 0).all()
    assert int(action.min()) >= 0 and int(action.max()) < ho.A_FULL
    stats, dead = ho.chi2_per_group(action, z)
    print(f"one launch of {n} rows: chi2 per vector"
          f" {[round(s, 2) for s in stats]}, limit {limit:.2f}; dead cells"
          f" drawn: {dead}")
    assert dead == 0, "an action at logit -40 was drawn"
    assert max(stats) < limit, stats

    # Neighbouring rows on the two-action uniform vector.
    g2 = dict(_vector_heads(torch.zeros(4, 2)), x=_one_hot_rows(n))
    a2, l2, _ = _heads(g2, n, greedy=False, seed=-12345, rows=n)
    assert (l2 == 0).all()
    a2 = a2.numpy()
    agree, pairs, sigma = ho.agreement(a2[1:], a2[:-1])
    ones = int(a2.sum())
    print(f"adjacent rows agreeing: {agree}, expected {pairs / 2} +-"
          f" {sigma:.1f}; ones: {ones}")
    assert abs(agree - pairs / 2) <= 5 * sigma
    assert abs(ones - n / 2) <= 5 * n ** 0.5 / 2


def test_draw_distribution_across_launches_seeded_as_the_runner_does():
    z = ho.four_logit_vectors()
    limit = ho.chi2_limit()
    rows, launches = ho.LAUNCH_ROWS, ho.N_LAUNCHES
    x = _one_hot_rows(rows)
    g18 = dict(_vector_heads(z), x=x)
    g2 = dict(_vector_heads(torch.zeros(4, 2)), x=x)
    want18 = z.repeat(rows // 4, 1)
    out18, out2 = _outputs(rows, ho.A_FULL), _outputs(rows, 2)
    a18, a2 = [], []
    for k in range(1, launches + 1):
        seed = ho.runner_seed(k)
        for g, out, acc in ((g18, out18, a18), (g2, out2, a2)):
            tb.heads_sample(g["x"], None, g["policy_w"], g["policy_b"],
                            g["base_w"], g["base_b"], rows, False, seed, *out)
            acc.append(out[0].clone())
        assert torch.equal(out18[1], want18) and (out2[1] == 0).all()
    a18, a2 = torch.stack(a18), torch.stack(a2).numpy()
    stats, dead = ho.chi2_per_group(a18.reshape(-1), z)
    print(f"{launches} launches of {rows} rows: pooled chi2 per vector"
          f" {[round(s, 2) for s in stats]}, limit {limit:.2f}; dead cells"
          f" drawn: {dead}")
    assert dead == 0, "an action at logit -40 was drawn"
    assert max(stats) < limit, stats
    # What one environment sees: its row in launch k and in launch k + 1.
    agree, pairs, sigma = ho.agreement(a2[1:], a2[:-1])
    print(f"consecutive launches agreeing: {agree}, expected {pairs / 2} +-"
          f" {sigma:.1f}")
    assert pairs == (launches - 1) * rows
    assert abs(agree - pairs / 2) <= 5 * sigma
    # ... and its neighbour in the same launch.
    agree, pairs, sigma = ho.agreement(a2[:, 1:], a2[:, :-1])
    assert abs(agree - pairs / 2) <= 5 * sigma


@pytest.mark.parametrize("with_rew", FORMS)
def test_seed_decides_the_actions_and_nothing_else(with_rew):
    b = ho.ROWS
    g = _gpu(ho.bounded_case(519, 18, with_rew))
    greedy = _heads(g, b)
    neg = ho.runner_seed(1)
    assert neg < 0
    first, again = (_heads(g, b, greedy=False, seed=neg) for _ in range(2))
    other = _heads(g, b, greedy=False, seed=ho.runner_seed(2))
    plus = _heads(g, b, greedy=False, seed=neg + (1 << 63))
    assert torch.equal(first[0], again[0])
    assert not torch.equal(first[0], other[0])
    # The sign bit is part of the seed: a negative one is not folded away.
    assert not torch.equal(first[0], plus[0])
    for out in (first, again, other, plus):
        assert torch.equal(out[1], greedy[1])
        assert torch.equal(out[2], greedy[2])
        assert ((out[0][:b] >= 0) & (out[0][:b] < 18)).all()
        _assert_pad_rows_kept(out, b)
    # The draws differ from the argmax somewhere: they are draws.
    assert not torch.equal(first[0], greedy[0])


# ---- gather_obs ----

REWARDS = (-2.5, 1.0, -0.0, float("inf"), -1.0, 0.0, float("-inf"), 1.5, 0.3,
           -0.7)
DONES = (0, 1, 2, 255)


def _slabs(slots, fsz):
    g = torch.Generator().manual_seed(slots * 1000003 + fsz)
    frames = torch.randint(0, 256, (slots, 1, fsz // 16, 16),
                           dtype=torch.uint8, generator=g).pin_memory()
    rew = torch.tensor([REWARDS[i % len(REWARDS)] for i in range(slots)])
    done = torch.tensor([DONES[(i // 3) % 4] for i in range(slots)],
                        dtype=torch.uint8)
    return frames, rew.pin_memory(), done.pin_memory()


def _ids(slots, b):
    """A shuffled subset with one id repeated; with enough slots, every
    special reward and done byte is among them."""
    g = torch.Generator().manual_seed(slots + b)
    must = list(range(min(12, b - 1)))
    rest = [i for i in torch.randperm(slots, generator=g).tolist()
            if i not in must][:b - 1 - len(must)]
    ids = must + rest
    ids.append(ids[1])
    order = torch.randperm(b, generator=g).tolist()
    ids = [ids[i] for i in order]
    assert len(ids) == b and len(set(ids)) == b - 1
    assert ids != sorted(ids)
    return torch.tensor([ids], dtype=torch.int32)


def _clip_host(r):
    """The host paths' expression, in float32."""
    r = r.astype(np.float32)
    return np.where(r < -1, np.float32(-1), np.where(r > 1, np.float32(1), r))


@pytest.mark.parametrize("slots,b,bp_pad", [(7, 5, 64), (300, 70, 128)])
@pytest.mark.parametrize("fsz", [16, 4096 + 16, 28224, 100800])
def test_gather_obs_matches_numpy(fsz, slots, b, bp_pad):
    frames, rew, done = _slabs(slots, fsz)
    ids = _ids(slots, b)
    sel = ids[0].long().numpy()
    shape = list(frames.shape[1:])
    want_f = frames.numpy()[sel]
    want_r = _clip_host(rew.numpy()[sel])
    want_nd = np.where(done.numpy()[sel] != 0, 0.0, 1.0).astype(np.float32)
    if slots >= 12:
        assert set(np.abs(rew.numpy()[sel])) >= {2.5, 1.0, 0.0, np.inf}
        assert set(done.numpy()[sel]) == set(DONES)
        assert np.signbit(rew.numpy()[sel][rew.numpy()[sel] == 0]).any()
    for bp, ids_in in ((b, ids), (bp_pad, ids), (bp_pad, ids.long())):
        out_f, out_r, out_nd = (t.cpu().numpy() for t in tb.gather_obs(
            frames, rew, done, ids_in, bp, shape))
        assert out_f.shape == (bp, *shape) and out_f.dtype == np.uint8
        assert out_r.shape == (bp, 1) and out_nd.shape == (bp,)
        assert np.array_equal(out_f[:b], want_f)
        assert np.array_equal(out_r[:b, 0].view(np.int32),
                              want_r.view(np.int32))
        assert np.array_equal(out_nd[:b], want_nd)
        # Pad rows: zero frames, reward +0.0, not done.
        assert not out_f[b:].any()
        assert not out_r[b:].view(np.int32).any()
        assert (out_nd[b:] == 1).all()


# ---- host checks ----


def _raises(kernel, fn):
    with pytest.raises(RuntimeError, match=kernel):
        fn()


def test_heads_host_checks_raise_before_launch():
    D, A, b = 65, 6, 5
    case = ho.bounded_case(D, A, True)
    g = _gpu(case)
    out = _outputs(b + 3, A)

    def call(b=b, greedy=True, seed=0, out=out, **kw):
        a = dict(g, **kw)
        tb.heads_sample(a["x"], a["rew"], a["policy_w"], a["policy_b"],
                        a["base_w"], a["base_b"], b, greedy, seed, *out)

    names = ("x", "rew", "policy_w", "policy_b", "base_w", "base_b")
    bad = []
    for name in names:
        t = g[name]
        bad.append({name: case[name]})           # on the CPU
        bad.append({name: t.double()})           # not f32
    bad.append({"x": g["x"].t().contiguous().t()})            # x strided
    bad.append({"rew": g["rew"].repeat_interleave(2)[::2]})   # rew strided
    bad.append({"policy_w": g["policy_w"].t().contiguous().t()})
    bad.append({"base_w": g["base_w"].repeat(1, 2)[:, ::2]})
    bad.append({"policy_b": g["policy_b"].repeat_interleave(2)[::2]})
    bad.append({"policy_b": torch.zeros(A + 1).cuda()})       # not A
    bad.append({"policy_b": torch.zeros(A - 1).cuda()})
    bad.append({"base_b": torch.zeros(2).cuda()})             # not 1
    bad.append({"base_b": torch.zeros(0).cuda()})
    bad.append({"base_w": g["base_w"].repeat(2, 1)})          # two rows
    bad.append({"policy_w": torch.zeros(0, D + 1).cuda(),     # A = 0
                "policy_b": torch.zeros(0).cuda()})
    bad.append({"policy_w": torch.zeros(65, D + 1).cuda(),    # A = 65
                "policy_b": torch.zeros(65).cuda()})
    bad.append({"policy_w": g["policy_w"][:, :D].contiguous()})  # not Dc
    bad.append({"base_w": g["base_w"][:, :D].contiguous()})
    bad.append({"rew": None})                    # weights are for [x, rew]
    bad.append({"x": g["x"][:b - 1]})            # fewer rows than b
    bad.append({"rew": g["rew"][:b - 1].contiguous()})
    bad.append({"x": g["x"][0]})                 # not [n, D]
    for kw in bad:
        _raises("heads_sample", lambda: call(**kw))
    _raises("heads_sample", lambda: call(b=0))
    _raises("heads_sample", lambda: call(b=-1))
    # A core beyond the LDS limit, whatever the device's is.
    wide = 1 << 20
    _raises("heads_sample", lambda: call(
        x=torch.zeros(b, wide).cuda(), rew=None,
        policy_w=torch.zeros(A, wide).cuda(),
        base_w=torch.zeros(1, wide).cuda()))
    # Outputs: pinned, typed, long enough.
    for i, t in ((0, out[0].clone()), (1, out[1].clone()), (2, out[2].clone()),
                 (0, out[0].int().pin_memory()),
                 (1, out[1].double().pin_memory()),
                 (0, out[0][:b - 1]), (1, out[1][:b - 1]), (2, out[2][:b - 1]),
                 (1, torch.zeros(b, A + 1).pin_memory())):
        wrong = list(out)
        wrong[i] = t
        _raises("heads_sample", lambda: call(out=tuple(wrong)))
    torch.cuda.synchronize()
    # Nothing ran: every output still holds the sentinel.
    _assert_pad_rows_kept(out, 0)
    # The unmodified call is accepted, in both forms.
    call()
    (ref_l, ref_b), (s_l, s_b) = ho.reference(case)
    assert not ho.judge("bounded", out[1][:b], out[2][:b],
                        (ref_l[:b], ref_b[:b]), (s_l[:b], s_b[:b]), K)[0]
    _assert_pad_rows_kept(out, b)
    only = _gpu(ho.bounded_case(D, A, False))
    call(**only)


def test_gather_obs_host_checks_raise_before_launch():
    slots, fsz, b, bp = 7, 4112, 5, 64
    frames, rew, done = _slabs(slots, fsz)
    ids = _ids(slots, b)
    shape = list(frames.shape[1:])

    def call(frames=frames, rew=rew, done=done, ids=ids, bp=bp, shape=shape):
        return tb.gather_obs(frames, rew, done, ids, bp, shape)

    odd = torch.zeros(slots, 1, 1, 24, dtype=torch.uint8).pin_memory()
    bad = [
        dict(frames=odd, shape=[1, 1, 24]),                  # fsz % 16
        dict(shape=[]),                                      # fsz = 1
        dict(frames=frames.to(torch.int8).pin_memory()),     # not u8
        dict(frames=frames.clone()),                         # not pinned
        dict(frames=frames.cuda()),                          # not on the host
        dict(rew=rew.double().pin_memory()),                 # not f32
        dict(rew=rew.clone()),
        dict(done=done.bool().pin_memory()),                 # not u8
        dict(done=done.clone()),
        dict(rew=torch.zeros(slots + 1).pin_memory()),       # slot counts
        dict(done=torch.zeros(slots - 1, dtype=torch.uint8).pin_memory()),
        dict(frames=torch.zeros(slots - 1, *shape,
                                dtype=torch.uint8).pin_memory()),
        dict(shape=[1, fsz // 16 - 1, 16]),                  # not the slab's
        dict(ids=torch.zeros(1, 0, dtype=torch.int32)),      # b = 0
        dict(bp=b - 1),                                      # b > bp
        dict(ids=ids.float()),                               # dtype
        dict(ids=ids.cuda()),
    ]
    for at in (0, b - 1):
        for value in (slots, -1, 1 << 20):
            stray = ids.clone()
            stray[0, at] = value
            bad.append(dict(ids=stray))
            bad.append(dict(ids=stray.long()))
    wide = ids.long()
    wide[0, 2] = (1 << 32) + 1  # in range only if cut to 32 bits
    bad.append(dict(ids=wide))
    for kw in bad:
        _raises("gather_obs", lambda: call(**kw))
    torch.cuda.synchronize()
    # The unmodified call is accepted afterwards, the last slot included.
    last = ids.clone()
    last[0, 0] = slots - 1
    out_f, _, _ = call(ids=last)
    assert torch.equal(out_f[:b].cpu(), frames[last[0].long()])
