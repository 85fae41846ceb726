"""Float64 reference, case tables, sampler statistics and a numpy model of
the Gumbel draw for heads_sample_kernel (runtime/csrc/runtime_kernels.hip).

The heads are two linear maps of one core vector per request,

    logits[r, a] = sum_i core[r, i] * policy_w[a, i] + policy_b[a]
    baseline[r]  = sum_i core[r, i] * base_w[0, i]   + base_b[0]

with core = [x, reward] (the stateless agent, Dc = D + 1) or x alone (the
recurrent tail, Dc = D). reference() evaluates both in float64 and returns,
per element, the sum S of the magnitudes that enter it, which is what a
float32 evaluation's rounding error scales with.

Two comparison rules, as for the conv kernels (conv_oracle.py):

  exact    small-integer operands: every partial sum is an integer far below
           2^24, so float32 gives the same answer in any summation order and
           the kernel must equal the reference bit for bit.
  bounded  random float32 operands: |got - ref| <= K * 2^-24 * S per element,
           K = 4 r with r the error of a plain float32 F.linear on the CPU
           against float64 over the same cases (cpu_float32_ratio()).

tests/test_heads_oracle.py checks the tables and that both rules and every
statistic reject what a subtly wrong kernel would produce, without a GPU;
tests/test_serve_heads_gpu.py runs the kernel against them.
"""

import functools

import numpy as np
import torch
import torch.nn.functional as F

EPS32 = 2.0 ** -24

# Lengths of x: a core below one lane stride of 64, at a stride boundary and
# one past it (with and without the reward), the shallow and the deep fc
# widths and the LSTM width.
D_VALUES = (1, 63, 64, 65, 256, 512, 519)
# A + 1 output rows are dealt over 4 waves: fewer rows than waves, and 17
# rounds of which the last is cut.
A_VALUES = (1, 6, 18, 64)
B_VALUES = (1, 5, 70, 300)
ROWS = max(B_VALUES)
DEAD_OUT = 4  # action a is dead (zero weights, zero bias) when a % 4 == 1

CPU_RATIO = 3.92  # r, measured by cpu_float32_ratio(): 3.913 at D = 64, A = 64
K = 4 * CPU_RATIO


def _gen(*key):
    return torch.Generator().manual_seed(
        sum((i + 1) * ord(ch) for i, ch in enumerate("/".join(map(str, key)))))


def core_of(x, rew):
    """[x, rew] or x alone, as the kernel stages it in LDS."""
    if rew is None:
        return x
    return torch.cat([x, rew.reshape(-1, 1).to(x.dtype)], 1)


def heads(core, policy_w, policy_b, base_w, base_b, absolute=False):
    """(logits, baseline) in float64; with `absolute`, the sums S of the
    magnitudes of every term instead."""
    ops = [t.double() for t in (core, policy_w, policy_b, base_w, base_b)]
    if absolute:
        ops = [t.abs() for t in ops]
    core, policy_w, policy_b, base_w, base_b = ops
    logits = core @ policy_w.t() + policy_b
    baseline = (core @ base_w.t() + base_b).reshape(-1)
    return logits, baseline


def reference(case):
    """Float64 (logits, baseline) and their S for a case dict."""
    core = core_of(case["x"], case["rew"])
    w = (case["policy_w"], case["policy_b"], case["base_w"], case["base_b"])
    return heads(core, *w), heads(core, *w, absolute=True)


# ---- case tables ----


def _zero_a_sum(x, fixed, w, bias, g):
    """Moves entries of the integer row x (values 0..4) one step at a time
    until x . w + fixed + bias == 0. Terminates for w[0] == -1 and
    1 <= bias <= 2, |fixed| <= 1: while the sum is off, some entry can move
    it towards zero (see tests/test_heads_oracle.py)."""
    t = int(x @ w) + fixed + bias
    order = torch.randperm(x.numel(), generator=g).tolist()
    while t != 0:
        step = -1 if t > 0 else 1  # what the sum has to change by
        for j in order:
            wj = int(w[j])
            if wj == step and x[j] < 4:
                x[j] += 1
                break
            if wj == -step and x[j] > 0:
                x[j] -= 1
                break
        else:  # pragma: no cover
            raise AssertionError("no entry left to move")
        t += step
    return x


@functools.lru_cache(maxsize=None)
def exact_case(D, A, with_rew):
    """Small-integer operands, float32, shared and never modified: x in
    {0..4} (about half zeros, as a post-ReLU fc output), reward in
    {-1, 0, 1}, weights in {-1, 0, 1} with one action in four dead, integer
    biases. Rows r % 4 == 0 are moved until their baseline is exactly zero
    and rows r % 4 == 2 until the logit of action 0 is, so that both outputs
    hold zeros the kernel has to compute; odd rows are redrawn until core and
    outputs differ from both neighbours'."""
    g = _gen("exact", D, A, with_rew)
    Dc = D + 1 if with_rew else D
    ri = lambda lo, hi, *s: torch.randint(lo, hi + 1, s, generator=g)  # noqa: E731
    policy_w = ri(-1, 1, A, Dc)
    base_w = ri(-1, 1, 1, Dc)
    policy_w[0, 0] = base_w[0, 0] = -1
    if with_rew:  # the reward's column is live in both heads
        policy_w[:, D] = ri(0, 1, A) * 2 - 1
        base_w[0, D] = 1
    policy_b = ri(-3, 3, A)
    policy_b[0] = 2
    base_b = torch.tensor([1])
    dead = torch.arange(A) % DEAD_OUT == 1
    policy_w[dead] = 0
    policy_b[dead] = 0
    rew = ri(-1, 1, ROWS) if with_rew else None

    def draw_row():
        return ri(0, 4, D) * ri(0, 1, D)

    def outputs(r, row):
        fixed_p = rew[r] * policy_w[:, D] if with_rew else 0
        fixed_b = int(rew[r] * base_w[0, D]) if with_rew else 0
        return (policy_w[:, :D] @ row + fixed_p + policy_b,
                int(base_w[0, :D] @ row) + fixed_b + int(base_b))

    x = torch.zeros(ROWS, D, dtype=torch.int64)
    for r in range(0, ROWS, 2):
        fixed = int(rew[r]) if with_rew else 0
        if r % 4 == 0:
            x[r] = _zero_a_sum(draw_row(), fixed * int(base_w[0, D])
                               if with_rew else 0, base_w[0, :D],
                               int(base_b), g)
        else:
            x[r] = _zero_a_sum(draw_row(), fixed * int(policy_w[0, D])
                               if with_rew else 0, policy_w[0, :D],
                               int(policy_b[0]), g)
    for r in range(1, ROWS, 2):
        near = [outputs(n, x[n]) for n in (r - 1, r + 1) if n < ROWS]
        for _ in range(1000):
            row = draw_row()
            lo, ba = outputs(r, row)
            if all(not torch.equal(lo, nl) and ba != nb for nl, nb in near):
                break
        else:  # pragma: no cover
            raise AssertionError("no row differs from its neighbours")
        x[r] = row
    f = lambda t: None if t is None else t.float()  # noqa: E731
    return dict(x=f(x), rew=f(rew), policy_w=f(policy_w), policy_b=f(policy_b),
                base_w=f(base_w), base_b=f(base_b))


@functools.lru_cache(maxsize=None)
def bounded_case(D, A, with_rew):
    """Random float32 operands, shared and never modified: x as a post-ReLU
    fc output (with the reward) or as an LSTM's h in (-1, 1) (without),
    rewards clipped to [-1, 1] with both ends present, weights at the scale
    of the model's initialisation."""
    g = _gen("bounded", D, A, with_rew)
    Dc = D + 1 if with_rew else D
    rn = lambda *s: torch.randn(*s, generator=g)  # noqa: E731
    k = 1.0 / Dc ** 0.5
    if with_rew:
        x = rn(ROWS, D).clamp_min(0.0)
        rew = (rn(ROWS) * 1.5).clamp(-1, 1)
        assert bool((rew == 1).any()) and bool((rew == -1).any())
    else:
        x = torch.tanh(rn(ROWS, D))
        rew = None
    return dict(x=x, rew=rew, policy_w=rn(A, Dc) * k, policy_b=rn(A) * k,
                base_w=rn(1, Dc) * k, base_b=rn(1) * k)


def case(kind, D, A, with_rew):
    return (exact_case if kind == "exact" else bounded_case)(D, A, with_rew)


# ---- the two comparison rules ----


def exact_mismatch(got, ref, what):
    """None if `got` equals `ref` exactly, else a message naming the output
    and the first differing row."""
    got = got.detach().cpu().double()
    if got.shape != ref.shape:
        return f"{what}: shape {tuple(got.shape)} != {tuple(ref.shape)}"
    if torch.equal(got, ref):
        return None
    bad = (got != ref).nonzero()
    i = tuple(int(v) for v in bad[0])
    return (f"{what}: {bad.shape[0]} of {ref.numel()} elements differ, first"
            f" at row {i[0]}, index {i}: got {float(got[i])!r}, want"
            f" {float(ref[i])!r}")


def bound_excess(got, ref, s, k, what):
    """(message or None, ratio): the largest |got - ref| in units of
    2^-24 * S, and a message naming output and row if it exceeds k."""
    got = got.detach().cpu().double()
    if got.shape != ref.shape:
        return (f"{what}: shape {tuple(got.shape)} != {tuple(ref.shape)}",
                float("inf"))
    err = (got - ref).abs()
    err = torch.where(torch.isnan(err), torch.full_like(err, float("inf")),
                      err)
    unit = EPS32 * s
    ratio = torch.where(unit > 0, err / unit.clamp_min(1e-300),
                        torch.where(err > 0, torch.full_like(err, float("inf")),
                                    torch.zeros_like(err)))
    worst = float(ratio.max())
    if worst <= k:
        return None, worst
    i = tuple(int(v) for v in (ratio == ratio.max()).nonzero()[0])
    return (f"{what}: {int((ratio > k).sum())} elements over the bound, worst"
            f" at row {i[0]}, index {i}: got {float(got[i])!r}, want"
            f" {float(ref[i])!r}, S {float(s[i]):.4g}, ratio {worst:.3g} >"
            f" K = {k:.3g}"), worst


def judge(kind, got_logits, got_baseline, refs, s, k=None):
    """(messages of the outputs that fail, largest bounded ratio)."""
    k = K if k is None else k
    bad, worst = [], 0.0
    for what, got, ref, ss in (("logits", got_logits, refs[0], s[0]),
                               ("baseline", got_baseline, refs[1], s[1])):
        if kind == "exact":
            msg = exact_mismatch(got, ref, what)
        else:
            msg, ratio = bound_excess(got, ref, ss, k, what)
            worst = max(worst, ratio)
        if msg is not None:
            bad.append(msg)
    return bad, worst


def cpu_float32_ratio():
    """r: the largest |f32 - f64| / (2^-24 * S) of a plain float32 F.linear
    on the CPU over the bounded cases of every D, A and core form."""
    worst = 0.0
    for D in D_VALUES:
        for A in A_VALUES:
            for with_rew in (True, False):
                c = bounded_case(D, A, with_rew)
                refs, s = reference(c)
                core = core_of(c["x"], c["rew"])
                got = (F.linear(core, c["policy_w"], c["policy_b"]),
                       F.linear(core, c["base_w"], c["base_b"]).reshape(-1))
                for g32, ref, ss in zip(got, refs, s):
                    worst = max(worst, float(((g32.double() - ref).abs()
                                              / (EPS32 * ss)).max()))
    return worst


# ---- wrong heads: what a subtly wrong kernel would return ----


def broken_heads(case, fault):
    """(logits, baseline) in float32 of a kernel with one fault:
    'reward_at_0'    the reward stored at core[0] instead of core[D];
    'base_from_policy' the baseline's dot product taken with policy_w row 0;
    'tail_dropped'   the core cut to 64 * floor(Dc / 64) elements;
    'no_bias'        both biases dropped."""
    x, rew = case["x"], case["rew"]
    core = core_of(x, rew).clone()
    pw, pb, bw, bb = (case[k] for k in ("policy_w", "policy_b", "base_w",
                                        "base_b"))
    if fault == "reward_at_0":
        core[:, 0] = rew
        core[:, -1] = 0
    elif fault == "base_from_policy":
        bw = pw[:1]
    elif fault == "tail_dropped":
        core[:, core.shape[1] // 64 * 64:] = 0
    elif fault == "no_bias":
        pb, bb = torch.zeros_like(pb), torch.zeros_like(bb)
    else:  # pragma: no cover
        raise ValueError(fault)
    logits, baseline = heads(core, pw, pb, bw, bb)
    return logits.float(), baseline.float()


# ---- sampler statistics (shared with tests/test_learner_kernels_gpu.py) ----

A_FULL = 18
DEAD = ((0, 17), (3, 9), (16, 17), (0, 1))  # the two -40 entries per vector
N_DRAWS = 200_000
N_LAUNCHES, LAUNCH_ROWS = 500, 400
GOLDEN = 0x9E3779B97F4A7C15  # InferenceRunner::next_seed()'s multiplier


@functools.lru_cache(maxsize=None)
def four_logit_vectors():
    """Four different 18-action vectors: 16 live logits in [-0.9, 0.9], so
    every live probability is at least e^-1.8/16 > 0.01, and two at -40."""
    g = torch.Generator().manual_seed(40)
    z = torch.rand(4, A_FULL, generator=g) * 1.8 - 0.9
    for k, dead in enumerate(DEAD):
        z[k, list(dead)] = -40.0
    return z


def chi2_limit():
    from scipy.stats import chi2

    return float(chi2.ppf(1 - 1e-6, A_FULL - 2 - 1))


def chi2_per_group(actions, z):
    """Pearson chi-square over the 16 live cells of each of the four
    interleaved groups (row r holds vector r % 4), and the number of draws
    of dead cells."""
    p = torch.softmax(z.double(), -1).numpy()
    actions = actions.numpy()
    stats, dead_draws = [], 0
    for k in range(4):
        counts = np.bincount(actions[k::4], minlength=A_FULL)
        n = counts.sum()
        live = [j for j in range(A_FULL) if j not in DEAD[k]]
        dead_draws += int(counts[list(DEAD[k])].sum())
        pk = p[k, live] / p[k, live].sum()  # dead mass is ~1e-17
        expected = n * pk
        assert expected.min() >= 500
        stats.append(float(((counts[live] - expected) ** 2 / expected).sum()))
    return stats, dead_draws


def agreement(a, b):
    """(pairs that agree, pairs, sigma) of two equally long draws from the
    two-action uniform vector: independent draws agree in half the pairs,
    with a standard deviation of sqrt(pairs) / 2."""
    a, b = np.asarray(a), np.asarray(b)
    assert a.shape == b.shape
    return int((a == b).sum()), a.size, a.size ** 0.5 / 2


def agreement_ok(a, b):
    agree, n, sigma = agreement(a, b)
    return abs(agree - n / 2) <= 5 * sigma


def runner_seed(k):
    """The k-th seed of a serving runner (k = 1, 2, ...) as the int64 the
    kernel's launcher takes: k * GOLDEN mod 2^64, reinterpreted as signed."""
    v = (k * GOLDEN) % (1 << 64)
    return v - (1 << 64) if v >= (1 << 63) else v


# ---- a numpy model of the kernel's draw ----

ONE_BELOW = np.nextafter(np.float32(1), np.float32(0))
BROKEN_SAMPLERS = ("neg_log", "last_never", "rows_share", "seed_shared")


def model_bits(seed, rows, A):
    """32 random bits per row and action, one stream per (seed, row) in
    effect: what philox gives the kernel, from numpy's generator."""
    rng = np.random.default_rng(seed % (1 << 64))
    return rng.integers(0, 1 << 32, size=(rows, A), dtype=np.uint32)


def model_draw(logits, bits, fault=None):
    """The kernel's draw in float32 numpy: u = (v + 1) * 2^-32 as
    hiprand_uniform rounds it, capped at the largest float below 1;
    g = z - log(-log(u)); the first index of the largest g. `fault` is one
    of BROKEN_SAMPLERS ('seed_shared' is a fault of the caller's seeds and
    draws like a correct sampler here)."""
    z = np.asarray(logits, dtype=np.float32)
    if fault == "rows_share":  # row r + 1 reads row r's stream
        bits = bits[np.arange(bits.shape[0]) // 2 * 2]
    p32 = np.float32(2.0 ** -32)
    u = np.minimum(p32 + bits.astype(np.float32) * p32, ONE_BELOW)
    assert u.dtype == np.float32 and float(u.min()) > 0
    if fault == "neg_log":
        g = z - np.log(u)
    else:
        g = z - np.log(-np.log(u))
    assert g.dtype == np.float32
    if fault == "last_never":
        g = g[:, :-1]
    return np.argmax(g, axis=1)


def model_one_launch(fault=None, seed=7):
    """(actions over N_DRAWS rows of the four interleaved vectors, actions
    over N_DRAWS rows of the two-action uniform vector) of one launch."""
    z = four_logit_vectors().numpy()
    a18 = model_draw(np.tile(z, (N_DRAWS // 4, 1)),
                     model_bits(seed, N_DRAWS, A_FULL), fault)
    a2 = model_draw(np.zeros((N_DRAWS, 2), np.float32),
                    model_bits(seed + 1, N_DRAWS, 2), fault)
    return a18, a2


def model_launches(fault=None):
    """The same two draws as N_LAUNCHES launches of LAUNCH_ROWS rows seeded
    as the runner seeds them: arrays [N_LAUNCHES, LAUNCH_ROWS]."""
    z = np.tile(four_logit_vectors().numpy(), (LAUNCH_ROWS // 4, 1))
    z2 = np.zeros((LAUNCH_ROWS, 2), np.float32)
    a18, a2 = [], []
    for k in range(1, N_LAUNCHES + 1):
        seed = runner_seed(1 if fault == "seed_shared" else k)
        a18.append(model_draw(z, model_bits(seed, LAUNCH_ROWS, A_FULL), fault))
        a2.append(model_draw(z2, model_bits(seed ^ 1, LAUNCH_ROWS, 2), fault))
    return np.stack(a18), np.stack(a2)


def sampler_verdicts(one_launch, launches):
    """Every statistic of the GPU tests on given draws: a dict of name ->
    passed. one_launch and launches are the pairs model_one_launch() and
    model_launches() return."""
    z = four_logit_vectors()
    limit = chi2_limit()
    a18, a2 = one_launch
    stats, dead = chi2_per_group(torch.from_numpy(a18), z)
    l18, l2 = launches
    lstats, ldead = chi2_per_group(torch.from_numpy(l18.reshape(-1)), z)
    return dict(
        chi2=max(stats) < limit,
        dead=dead == 0 and ldead == 0,
        neighbours=agreement_ok(a2[1:], a2[:-1]),
        chi2_launches=max(lstats) < limit,
        launch_neighbours=agreement_ok(l2[1:], l2[:-1]),
    )
