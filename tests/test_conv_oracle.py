"""The float64 conv references (tests/helpers/conv_oracle.py) checked on their
own, without a GPU: that the integer cases of
tests/test_conv_mfma_exact_gpu.py are exact in the kernels' arithmetic and are
not tests of zeros, that the packed layouts are the ones autograd's gradients
map to, and that the two comparison rules reject what a subtly wrong kernel
would compute.
"""

import os
import sys

import pytest
import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)),
                                "helpers"))

import conv_oracle as co  # noqa: E402

from torchbeast_amd.ops import functional as tbf  # noqa: E402

TWO24 = 2.0 ** 24


def _is_int(t):
    return bool((t == t.round()).all())


def _covered(t, what):
    """Between 20 % and 80 % of the elements are nonzero."""
    share = float((t != 0).double().mean())
    assert 0.2 <= share <= 0.8, f"{what}: {share:.3f} of elements nonzero"


def _six_distinct(t, what):
    """Any six consecutive samples are pairwise distinct."""
    flat = t.reshape(t.shape[0], -1)
    for lag in range(1, min(6, flat.shape[0])):
        same = (flat[lag:] == flat[:-lag]).all(1)
        assert not bool(same.any()), f"{what}: samples {lag} apart coincide"


def _trunk_ns(geom):
    ns = {n for g, n in co.FWD_CASES + co.DGRAD3_CASES + co.DGRAD2_CASES
          if g == geom and n < 1023}
    for cases in co.WGRAD_CASES.values():
        ns |= {n for g, n in cases if g == geom}
    # and the rotated base of the large batches, and the end-to-end cases
    return sorted(ns | ({co.ROTATE, 6} if geom == "84" else {2}))


# ---- range, coverage and distinct-neighbour conditions ----


@pytest.mark.parametrize("geom", list(co.GEOM))
def test_integer_chain_is_exact_and_covered(geom):
    ch = co.int_chain(geom)
    assert max(_trunk_ns(geom)) <= co.NMAX[geom]
    # Everything a kernel stores as bf16 is an integer of at most 256.
    for k in ("a1", "a2", "d3m", "d2", "d1"):
        assert _is_int(ch[k]) and float(ch[k].abs().max()) <= 256, k
    assert _is_int(ch["out3"]) and float(ch["out3"].max()) < TWO24
    assert set(ch["frames"].unique().tolist()) == {0, 255}
    assert torch.equal(co.frames_operand(ch["frames"]),
                       (ch["frames"] != 0).double())
    # Coverage for the samples of every case, ReLU masks included: a1, a2
    # and out3 are zero exactly where their layer's ReLU masks.
    for n in _trunk_ns(geom):
        for k in ("a1", "a2", "out3", "d3m", "d2", "d1"):
            _covered(ch[k][:n], f"{k}[:{n}]")
    for k in ("frames", "a1", "a2", "d3m", "d2", "d1", "d_out"):
        _six_distinct(ch[k], k)
    # The rotated batches: any six neighbours differ because the 7 do.
    assert co.ROTATE == 7 and all(co.ROTATE % sb for sb in (3, 6))
    # Sum of |terms| of every forward and dgrad element.
    s1, s2, s3 = (co.trunk_layer(i, ch[x], ch[w], ch[b], absolute=True)
                  for i, x, w, b in ((1, "frames", "w1p", "b1"),
                                     (2, "a1", "w2p", "b2"),
                                     (3, "a2", "w3p", "b3")))
    sd2 = co.sum_abs(co.conv_trunk_dgrad3, ch["d3m"], ch["w3r"], ch["a2"])
    sd1 = co.sum_abs(co.conv_trunk_dgrad2, ch["d2"], ch["w2r"], ch["a1"])
    for s in (s1, s2, s3, sd2, sd1):
        assert float(s.max()) < TWO24
    # dgrad3's mask has zeros and positives at every corner and inside.
    a2 = ch["a2"]
    for n in (1, 6):
        for yy, xx in ((0, 0), (0, -1), (-1, 0), (-1, -1), (4, 4)):
            at = a2[:n, yy, xx, :]
            assert bool((at == 0).any()) and bool((at > 0).any()), (n, yy, xx)


@pytest.mark.parametrize("layer", [1, 2, 3])
def test_integer_wgrad_cases_are_exact_and_covered(layer):
    for geom, n in co.WGRAD_CASES[layer]:
        dw, db = co.int_wgrad(geom, layer, n)
        s, sdb = co.int_wgrad(geom, layer, n, True)
        assert _is_int(dw) and _is_int(db)
        assert float(s.max()) < TWO24 and float(sdb.max()) < TWO24
        _covered(dw, f"dW{layer} {geom} N={n}")
        _covered(db, f"db{layer} {geom} N={n}")
        ci = co.GEOM[geom]["frame"][0] if layer == 1 else co.CO[layer - 1]
        kwc = co.KS[layer] * ci
        assert dw.shape == (co.KS[layer], co.CO[layer], co.kwcp(co.KS[layer],
                                                                 ci))
        assert not bool(dw[..., kwc:].any())


@pytest.mark.parametrize("geom,n", co.MASK_CASES)
def test_integer_mask_cases(geom, n):
    ops = co.int_ops("mask", geom, n)
    ref = co.entry_refs("mask", ops)["d3m"]
    assert bool((ops["out3"] == 0).any()) and _is_int(ref)
    assert float(ref.abs().max()) <= 256
    _covered(ops["out3"], "out3")
    _covered(ref, "d3m")
    _six_distinct(ref, "d3m")
    if n == 168:  # the grid of 2048 blocks of 256 threads wraps
        assert ref.numel() > 2048 * 256 and (ref.numel() - 3136) <= 2048 * 256


@pytest.mark.parametrize("geom", co.RESNET_GEOMS)
def test_integer_resnet_cases_are_exact_and_covered(geom):
    ci, hw, co_ = geom
    c = co.resnet_int_case(geom)
    ns = sorted({n for cases in (co.RESNET_FWD_CASES, co.RESNET_DGRAD_CASES,
                                 co.RESNET_WGRAD_CASES)
                 for g, n in cases if g == geom})
    assert max(ns) <= co.RESNET_NMAX[hw]
    x = c["x"]
    assert _is_int(x) and _is_int(c["dy"]) and float(x.abs().max()) <= 2
    for yy in (0, -1):  # corners and borders carry data
        for xx in (0, -1):
            assert bool((x[:, yy, xx, :] != 0).all())
    for border in (x[:, 0], x[:, -1], x[:, :, 0], x[:, :, -1]):
        _covered(border, "border")
    _six_distinct(x, "x")
    _six_distinct(c["dy"], "dy")
    for n in ns:
        kinds = ("fwd", "wgrad") if ci == 8 else ("fwd", "dgrad", "wgrad")
        for kind in kinds:
            ref = co.resnet_int_ref(geom, kind, n)
            s = co.resnet_int_ref(geom, kind, n, True)
            outs = (zip(ref, s, ("dW", "db")) if kind == "wgrad"
                    else [(ref, s, kind)])
            for r, ss, name in outs:
                assert _is_int(r) and float(ss.max()) < TWO24
                if name in ("fwd", "dgrad"):
                    assert float(r.abs().max()) <= 256
                _covered(r, f"{geom} {name} N={n}")
    if ci == 8:  # the end-to-end first conv sees 4 observation channels
        _, dw4, db4 = co.resnet_int_autograd(geom, 3, first_ci=4)
        assert _is_int(dw4)
        _covered(dw4, "first conv dw")
        _covered(db4, "first conv db")
    dw, _ = co.resnet_int_ref(geom, "wgrad", 1)
    assert dw.shape == (3, co_, co.kwcp(3, ci))
    assert not bool(dw[..., 3 * ci:].any())


# ---- layouts against plain autograd ----


@pytest.mark.parametrize("geom,n", [("84", 6), ("fr", 2)])
def test_trunk_layouts_match_autograd(geom, n):
    ch = co.int_chain(geom)
    grads = co.int_autograd(geom, n)
    for layer in (1, 2, 3):
        dwp, db = co.int_wgrad(geom, layer, n)
        ci = grads[2 * layer - 2].shape[1]
        dw = co.unpack_dw(dwp, ci, c_major=(layer == 1))
        assert torch.equal(dw, grads[2 * layer - 2]), f"dw{layer}"
        assert torch.equal(db, grads[2 * layer - 1]), f"db{layer}"
        assert torch.equal(co.pack_dw(dw, layer == 1), dwp)
    # The helper packs operands as the Python wrappers do.
    w1p, w2p, w3p = tbf._pack_trunk_weights(ch["w1"], ch["w2"], ch["w3"])
    assert torch.equal(w1p, ch["w1p"]) and torch.equal(w2p, ch["w2p"])
    assert torch.equal(w3p, ch["w3p"])
    assert torch.equal(co.unpack_w(ch["w2p"], 4, 32), ch["w2"].double())
    assert torch.equal(co.unpack_rot(ch["w3r"], 3, 64), ch["w3"].double())
    assert torch.equal(co.unpack_w1(ch["w1p"]), ch["w1"].double())


@pytest.mark.parametrize("geom", co.RESNET_GEOMS)
def test_resnet_layouts_match_autograd(geom):
    ci, hw, _ = geom
    c = co.resnet_int_case(geom)
    n = co.RESNET_NMAX[hw]
    dx, dw, db = co.resnet_int_autograd(geom, n)
    dwp, dbr = co.resnet_int_ref(geom, "wgrad", n)
    assert torch.equal(co.unpack_dw(dwp, ci, False), dw)
    assert torch.equal(dbr, db)
    assert torch.equal(co.nchw(co.resnet_int_ref(geom, "dgrad", n)), dx)
    y = F.conv2d(co.nchw(c["x"][:n]).double(), c["w"].double(),
                 c["b"].double(), padding=1)
    assert torch.equal(co.nchw(co.resnet_int_ref(geom, "fwd", n)), y)
    assert torch.equal(tbf._pack_resnet_weight(c["w"]), c["wp"])
    assert torch.equal(tbf._pack_resnet_weight(c["w"], rotate=True), c["wr"])


# ---- the comparison rules reject what a wrong kernel would compute ----

# entry -> (integer case, random-valued case)
MUTATION_CASES = {
    "fwd": (("84", 2), None),
    "conv1": (None, ("84", 3)),
    "conv2": (("84", 2), ("84", 3)),
    "conv3": (("fr", 2), ("84", 3)),
    "mask": (("84", 2), ("84", 168)),
    "dgrad3": (("84", 6), ("84", 6)),
    "dgrad2": (("84", 3), ("84", 3)),
    "wgrad1": (("84", 6), ("84", 6)),
    "wgrad2": (("84", 26), ("84", 26)),
    "wgrad3": (("84", 21), ("84", 21)),
    "rn_fwd": (((8, 84, 16), 3), ((32, 11, 32), 9)),
    "rn_dgrad": (((16, 42, 32), 3), ((32, 11, 32), 9)),
    "rn_wgrad": (((32, 11, 32), 9), ((32, 11, 32), 9)),
}


def _round_like_kernel(refs):
    """What a kernel without fault would store: bf16 or fp32 roundings."""
    return {k: (v.to(torch.bfloat16) if k in co.BF16_OUT else v.float())
            for k, v in refs.items()}


def _accepts(got, refs, s, exact):
    """The comparison of tests/test_conv_mfma_exact_gpu.py over all outputs:
    True if `got` would pass."""
    for k, ref in refs.items():
        if exact:
            bad = co.exact_mismatch(got[k], ref)
        else:
            bad, _ = co.bound_excess(got[k], ref, s[k], co.K,
                                     k in co.BF16_OUT)
        if bad is not None:
            return False
    return True


def _mutants(entry, ops, refs):
    """(name, outputs a wrong kernel would give) for every damage that
    applies to `entry`."""
    def through(m_ops):
        return _round_like_kernel(co.entry_refs(entry, m_ops))

    if entry == "mask":
        out3 = ops["out3"].clone()
        hit = ((out3 > 0) & (ops["d_out"] != 0)).nonzero()[-1]
        out3[tuple(hit)] = 0
        yield "mask bit", through(dict(ops, out3=out3))
        yield "neighbour", _round_like_kernel(co.mutate_neighbour_out(refs))
        return
    if entry in co.WEIGHT_KEY:
        yield "tap", through(co.mutate_tap(entry, ops))
        yield "neighbour", _round_like_kernel(co.mutate_neighbour_out(refs))
    else:
        yield "m row", through(co.mutate_m_row(entry, ops))
        yield "neighbour", through(co.mutate_neighbour_in(entry, ops))
    yield "edge column", through(co.mutate_edge(entry, ops))


@pytest.mark.parametrize("entry,exact", [
    pytest.param(e, x, id=f"{e}-{'integer' if x else 'random'}")
    for e, cases in MUTATION_CASES.items() for x in (True, False)
    if cases[0 if x else 1] is not None])
def test_comparison_rejects_mutants(entry, exact):
    case = MUTATION_CASES[entry][0 if exact else 1]
    ops = (co.int_ops if exact else co.rand_ops)(entry, *case)
    refs = co.entry_refs(entry, ops)
    s = None if exact else co.entry_refs(entry, ops, absolute=True)
    assert _accepts(_round_like_kernel(refs), refs, s, exact)
    seen = 0
    for name, got in _mutants(entry, ops, refs):
        assert not _accepts(got, refs, s, exact), f"{entry}: {name} passes"
        seen += 1
    assert seen >= 2


@pytest.mark.parametrize("entry,case", [("conv2", ("84", 3)),
                                        ("dgrad2", ("84", 3)),
                                        ("rn_fwd", ((32, 11, 32), 9))])
def test_bound_rejects_truncating_bf16_store(entry, case):
    """A store that chops the fp32 result to bf16 instead of rounding it is
    off by up to a whole bf16 ulp: the half ulp of the bound must catch it."""
    ops = co.rand_ops(entry, *case)
    refs = co.entry_refs(entry, ops)
    s = co.entry_refs(entry, ops, absolute=True)
    chopped = {k: (v.float().view(torch.int32) & -65536).view(torch.float32)
               for k, v in refs.items()}
    assert not _accepts(chopped, refs, s, exact=False)


def test_exact_mismatch_names_the_element():
    ref = torch.zeros(2, 3, dtype=torch.float64)
    got = ref.clone()
    got[1, 2] = 1
    assert "(1, 2)" in co.exact_mismatch(got, ref)
    assert co.exact_mismatch(ref.clone(), ref) is None


def test_cpu_float32_ratio_recorded():
    """r, from which K = 4 r is derived: float32 convolutions on the CPU
    against float64 over the random-valued cases."""
    worst = co.cpu_float32_ratio()
    print("float32 CPU vs float64, units of 2^-24*S:",
          {k: round(v, 3) for k, v in worst.items()},
          f"recorded r = {co.CPU_RATIO}, K = {co.K:.2f}")
    assert max(worst.values()) <= co.K
