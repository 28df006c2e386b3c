"""The per-sample kernels and both weight packers on weights that are NOT the one recipe every other test draws from.

synth.make_hot_weights gives dense Gaussian matrices, all weights of a layer in one binade or two, gains of 0.25-4, sigmoid_beta = 0.1: a wrong
bf16 tie rule, a lost carry, a flushed low part, a float norm sum, a gain read from the wrong row or two swapped elements of similar size all
stay below 1e-4 there.  synth.make_weight_family gives four other kinds of numbers:

  wide    magnitudes log-uniform over six decades per matrix; per row one fp32 subnormal (2^-130) and one value whose low bf16 part is subnormal
  ties    every weight and bias on, next to, or carrying over a bf16 rounding tie; the weight-norm fold multiplies by exactly 1
  sparse  90 % exact zeros (some -0.0), all-zero output rows and input columns, half the biases zero
  gains   weight_g log-uniform over [0.05, 30] per row (activations up to ~2e4), sigmoid_beta 0.5 / 0.02 / 1e-3 (below the 2e-3 clamp)

On the CPU: the fp64 oracle is finite on each family with 5-95 % of the samples valid and 5-95 % of those with alpha > 0, and each family has
the property it is named for; the host packer's fp32 stream holds, POSITION BY POSITION (slot tables of vanerf_layer_slots), the weight-norm
fold computed here in fp64 (2 ulp: root, quotient, product; no weight-norm: the same bits); the bf16x3 streams hold torch.bfloat16's
round-to-nearest-even of that value and of its remainder.  On an MI355X: the device packer gives the host packer's bits in both directions
(recipe -> family -> recipe), the three forward kernels and the fused backward meet the fp64 oracle on every family, non-finite weights
give non-finite outputs in both modes, and VANeRF follows a change of `precision`.

Bars.  wide / ties / sparse: the project's 1e-4 and the sigma check of tests/test_posed_source.py.  gains: no absolute number has a
derivation at activations of 1e4, so the bar comes from the oracle alone: E32 = per-output max |fp32 oracle - fp64 oracle| on the same
points, A = the largest fp64 pre-activation; fp32 kernel max(1e-4, 4 E32) (4: an MFMA chain sums in another order than torch's GEMM),
bf16x3 kernels max(1e-4, 4 E32 + 2^-15 A) (the dropped lo x lo product is 2^-16 of a product, twice that as headroom); sigma beta =
sigmoid(-alpha / beta) is 1 / (4 beta)-Lipschitz in alpha, so its bar is alpha's / (4 beta) with the HANDLE's clamped beta."""
import pytest
import torch

from oracle import vanerf_oracle as orc
from tests.test_oracle_fp64 import cast, reference
from tests.test_oracle_posed import decision_margins, mesh_queries, near_mesh_points, posed_frame
from vanerf_amd import synth

TOL = 1e-4
N_POINTS = 2000
FAMILIES = synth.WEIGHT_FAMILIES
WN = "weight_v"
_CPU = {}


def _family(name):
    """Per family, built once, CPU only: weights (seed 0), the pose-A frame, N_POINTS points near its mesh, the oracle's mesh queries and its
    per-sample pass in fp64 and fp32."""
    if name not in _CPU:
        sd = synth.make_weight_family(name, 0)
        frame = posed_frame("A", 3)
        pts = near_mesh_points(frame, N_POINTS, seed=2)
        q_sdf, q_vis, vert_vis = mesh_queries(frame, pts)
        r64 = reference(sd, frame, pts, q_sdf, q_vis, vert_vis)
        r32 = reference(sd, frame, pts, q_sdf, q_vis, vert_vis, dtype=torch.float32)
        _CPU[name] = dict(sd=sd, frame=frame, pts=pts, q_sdf=q_sdf, q_vis=q_vis, vert_vis=vert_vis, r64=r64, r32=r32)
    return _CPU[name]


def _matrices(sd):
    return [k for k in sd if k.startswith(synth.PACKED_PREFIXES) and k.endswith(("weight", WN))]


def _fold64(sd, key):
    """The folded matrix (rows, kin) of a packed entry in fp64: v g / ||v|| for a weight-norm direction, the matrix itself otherwise."""
    m = sd[key].reshape(sd[key].shape[0], -1).double()
    if key.endswith(WN):
        m = m * (sd[key[:-1] + "g"].reshape(-1, 1).double() / m.norm(2, dim=1, keepdim=True))
    return m


def _ordered(x):
    """fp32 -> int64 that counts representable numbers: |a - b| in ulps is |_ordered(a) - _ordered(b)|, subnormals and +-0 included."""
    b = x.contiguous().view(torch.int32).long()
    return torch.where(b < 0, -(b & 0x7fffffff), b)


def _bf16_parts(v):
    """(hi, lo) bit patterns (int64, 16 bits) of fp32 `v` by torch.bfloat16's round-to-nearest-even: hi = bf16(v), lo = bf16(v - hi)."""
    hi = v.to(torch.bfloat16)
    lo = (v - hi.float()).to(torch.bfloat16)
    return hi.view(torch.int16).long() & 0xffff, lo.view(torch.int16).long() & 0xffff


# ---------------------------------------------------------------------------------------------------------------------
# 1. the families (CPU)
# ---------------------------------------------------------------------------------------------------------------------
def test_families_rewrite_the_packed_entries_only():
    from vanerf_amd.model import VANeRF
    assert synth.PACKED_PREFIXES is VANeRF._PACKED_PREFIXES
    base = synth.make_full_weights(0)
    for name in FAMILIES:
        sd = synth.make_weight_family(name, 0)
        assert list(sd) == list(base)
        for k in sd:
            assert sd[k].shape == base[k].shape and sd[k].dtype == torch.float32, (name, k)
            if not k.startswith(synth.PACKED_PREFIXES):
                assert torch.equal(sd[k], base[k]), (name, k)
        again = synth.make_weight_family(name, 0)
        assert all(torch.equal(sd[k].view(torch.int32), again[k].view(torch.int32)) for k in sd)  # seeded: the same bits
    with pytest.raises(ValueError):
        synth.make_weight_family("dense", 0)
    with pytest.raises(ValueError):
        synth.make_weight_family("wide", 3)  # no tuned head bias for that seed


@pytest.mark.parametrize("name", FAMILIES)
def test_family_properties(name):
    """The fp64 oracle on the family: finite, 5-95 % valid samples, 5-95 % of them with alpha > 0, no point within 1e-5 of a validity decision,
    fp32 and fp64 agree on validity; and the family has the property it is named for."""
    c = _family(name)
    sd, r64 = c["sd"], c["r64"]
    valid = r64["valid"]
    out = orc.eval_func(cast(sd, torch.float64), r64["raw"][None], valid[None, :, None], 100.0)[0]
    assert torch.isfinite(r64["raw"]).all() and torch.isfinite(out).all()
    assert all(torch.isfinite(y).all() for _, y in r64["layers"].values())
    share = (out[valid, 0] > 0).float().mean().item()
    assert 0.05 < valid.float().mean() < 0.95 and 0.05 < share < 0.95, (valid.float().mean().item(), share)
    assert decision_margins(c["frame"], c["pts"])[0].min() > 1e-5 and torch.equal(c["r32"]["valid"], valid)
    A = max(y.abs().max().item() for _, y in r64["layers"].values())
    e32 = (c["r32"]["raw"].double() - r64["raw"]).abs().max(0)[0]
    print(f"{name}: valid {valid.float().mean().item():.3f}, alpha > 0 on {share:.3f} of them, largest pre-activation {A:.3e}, "
          f"fp32 oracle vs fp64 [sdf, rad, r, g, b] {[f'{e:.1e}' for e in e32.tolist()]}")
    mats = _matrices(sd)
    assert len(mats) == 20
    if name == "wide":
        for k in mats:
            m = sd[k].reshape(sd[k].shape[0], -1)
            sub, small = m.abs() == synth.WIDE_TINY[0], m.abs() == synth.WIDE_TINY[1]
            one = torch.ones(m.shape[0], dtype=torch.long)
            assert torch.equal(sub.sum(1), one) and torch.equal(small.sum(1), one), k  # the two planted magnitudes, once per row each
            assert 0 < synth.WIDE_TINY[0] < 2.0 ** -126 < synth.WIDE_TINY[1]
            rest = m.abs()[~sub & ~small]
            decades = torch.log10(rest.max() / rest.min()).item()
            assert decades <= synth.WIDE_DECADES and decades > synth.WIDE_DECADES - (2.0 if rest.numel() < 100 else 0.5), (k, decades)
            # their bf16 parts where no fold moves the value: a subnormal high part with a zero low part; a normal high part with a low part
            # that is subnormal and not zero
            if not k.endswith(WN):
                f = m.float()
                hi, lo = _bf16_parts(f[sub])
                assert ((hi & 0x7f80) == 0).all() and ((hi & 0x7f) != 0).all() and ((lo & 0x7fff) == 0).all(), k
                hi, lo = _bf16_parts(f[small])
                assert ((hi & 0x7f80) != 0).all() and ((lo & 0x7f80) == 0).all() and ((lo & 0x7f) != 0).all(), k
            else:  # folded: g / ||v|| moves both by a factor of order 1
                f = _fold64(sd, k).float()
                hi, lo = _bf16_parts(f[small])
                assert (((lo & 0x7f80) == 0) & ((lo & 0x7f) != 0)).float().mean() > 0.5, k
                assert (f[sub].abs() < 2.0 ** -126).float().mean() > 0.5 and (f[sub] != 0).all(), k
    elif name == "ties":
        kinds = torch.zeros(5, dtype=torch.long)  # exact tie (even lower neighbour, odd), tie -+ 1 ulp, carry
        total = 0
        for k in mats + [k for k in sd if k.startswith(synth.PACKED_PREFIXES) and k.endswith("bias")]:
            b = sd[k].reshape(-1).view(torch.int32).long()
            low, odd, ones = b & 0xffff, (b >> 16) & 1, ((b >> 16) & 0x7f) == 0x7f
            carry = ones & ((low == 0x8000) | (low == 0xffff))
            kinds += torch.stack([((low == 0x8000) & ~ones & (odd == 0)).sum(), ((low == 0x8000) & ~ones & (odd == 1)).sum(),
                                  ((low == 0x7fff) | (low == 0x8001)).sum(), carry.sum(), torch.tensor(0)])
            total += b.numel()
            assert ((low == 0x8000) | (low == 0x7fff) | (low == 0x8001) | carry).all(), k  # every value is one of the three kinds
            if k.endswith(WN):  # the fold is the identity: g = ||v|| as the packers compute it
                g = sd[k[:-1] + "g"].reshape(-1)
                assert torch.equal(g, synth._norm_as_packed(sd[k].reshape(g.numel(), -1)))
            hi, _ = _bf16_parts(sd[k].reshape(-1)[carry])
            assert (((hi >> 7) & 0xff) == ((b[carry] >> 23) & 0xff) + 1).all(), k  # rounding carried into the next exponent
        third = total // 3
        assert kinds[0] + kinds[1] + kinds[2] + kinds[3] == total
        assert abs(int(kinds[0] + kinds[1]) - third) < 0.02 * total and abs(int(kinds[2]) - third) < 0.02 * total and abs(int(kinds[3]) - third) < 0.02 * total
        assert kinds[0] > 0.1 * total and kinds[1] > 0.1 * total  # both parities of the lower neighbour
    elif name == "sparse":
        for k in mats:
            m = sd[k].reshape(sd[k].shape[0], -1)
            rows, cols = synth.sparse_zero_lines(m.shape, k.endswith(WN))
            zr, zc = int((m == 0).all(1).sum()), int((m == 0).all(0).sum())
            assert (zr, zc) == (rows, cols), (k, zr, zc)
            if m.numel() >= 2000:  # (a small matrix keeps a value in every other row and column: fewer zeros)
                assert abs((m == 0).float().mean().item() - synth.SPARSE_ZERO_SHARE) < 0.03, k
            assert rows == (0 if k.endswith(WN) or m.shape[0] == 2 else 1 if m.shape[0] == 3 else 2) and cols == 2, k
        every = torch.cat([sd[k].reshape(-1) for k in mats])
        neg0 = ((every == 0) & (every.view(torch.int32) < 0)).sum().item()
        assert neg0 > 1000 and ((every == 0) & (every.view(torch.int32) == 0)).sum().item() > 5 * neg0
        for k in [k for k in sd if k.startswith(synth.PACKED_PREFIXES) and k.endswith("bias")]:
            assert int((sd[k] == 0).sum()) == (sd[k].numel() + 1) // 2, k
    else:
        lo, hi = synth.GAINS_RANGE
        gs = torch.cat([sd[k].reshape(-1) for k in sd if k.endswith("weight_g")])
        assert gs.numel() == 504 and lo <= gs.min() < 2 * lo and hi / 2 < gs.max() <= hi and 0.5 < gs.median() < 3.0
        assert [synth.make_weight_family("gains", s)["sigmoid_beta"].item() for s in (0, 1, 2)] == [torch.tensor(b).item() for b in synth.GAINS_BETAS]
        assert synth.make_weight_family("gains", 0, sigmoid_beta=0.02)["sigmoid_beta"].item() == torch.tensor(0.02).item()
        assert A > 1e3  # activations have grown: the recipe's largest pre-activation is ~10


# ---------------------------------------------------------------------------------------------------------------------
# 2. the host packer against the matrices (CPU)
# ---------------------------------------------------------------------------------------------------------------------
def _layer_tables():
    """Per layer of the packed streams: parameter (kind, name), rows used, the slot -> input channel table (vanerf_layer_slots: -1 unused,
    -2 bias)."""
    from vanerf_amd import hip_backward as HB
    return [(spec, lay["n_out"], lay["slots"].long()) for lay, spec in zip(HB.layout()["layers"], HB.LAYER_PARAMS)]


def _layer_folded(sd, spec, n_out):
    """(W64 (n_out, kin) folded in fp64, bias fp32 or None, weight-norm?) of one layer."""
    kind, name = spec
    key = name if kind == "conv" else name + (".weight_v" if kind == "wn" else ".weight")
    return _fold64(sd, key)[:n_out], (None if kind == "conv" else sd[name + ".bias"][:n_out]), kind == "wn"


def _expected_f32(W64, bias, slots, nb):
    """The fp32 forward stream of one layer, float [T][64 lanes][nb] (layer_spec.h): lane (j, h) of k-step t and block ob holds
    W[32 ob + j][slot 2 t + h], the bias in a bias slot, +0.0 in an unused slot or beyond the layer's rows."""
    T, n_out = slots.numel() // 2, W64.shape[0]
    t, lane, ob = torch.meshgrid(torch.arange(T), torch.arange(64), torch.arange(nb), indexing="ij")
    o, k = ob * 32 + (lane & 31), slots[2 * t + (lane >> 5)]
    inside = o < n_out
    oc = o.clamp(max=n_out - 1)
    val = torch.where(k >= 0, W64[oc, k.clamp(min=0)], torch.zeros((), dtype=torch.float64))
    if bias is not None:
        val = torch.where(k == -2, bias.double()[oc], val)
    used = inside & (k != -1) & ((k >= 0) | (bias is not None))
    return torch.where(used, val, torch.zeros((), dtype=torch.float64)).reshape(-1), used.reshape(-1)


@pytest.mark.parametrize("name", FAMILIES + ("recipe",))
def test_fp32_stream_holds_the_fp64_fold_position_by_position(name):
    """stream_host(sd, 0) against W = v g / ||v|| computed here in fp64 and rounded to fp32, every word of every layer at its position: the
    same bits where the layer has no weight-norm and in every bias and padding word (+0.0), within 2 ulp where it has (the packers round the
    root, the quotient and the product).  On 'ties' the fold is the identity: the same bits there too."""
    from vanerf_amd import renderer as R
    sd = synth.make_full_weights(0) if name == "recipe" else _family(name)["sd"]
    stream, offs = R.pack_weights_host(sd)
    assert torch.equal(stream.view(torch.int32), R.stream_host(sd, 0))
    offs = list(offs) + [stream.numel() - 2 * 64 * 4]
    assert torch.equal(stream[offs[-1]:].view(torch.int32), torch.zeros(512, dtype=torch.int32))  # the slack behind the last layer
    worst = 0
    for l, (spec, n_out, slots) in enumerate(_layer_tables()):
        got = stream[offs[l]:offs[l + 1]]
        nb = got.numel() // (slots.numel() // 2 * 64)
        assert nb * (slots.numel() // 2) * 64 == got.numel() and n_out <= 32 * nb, l
        W64, bias, wn = _layer_folded(sd, spec, n_out)
        want64, used = _expected_f32(W64, bias, slots, nb)
        want = want64.float()
        assert int(used.sum()) >= W64.numel(), l  # every element of the matrix has a place (some inputs are gathered twice)
        if wn:
            ulps = (_ordered(got) - _ordered(want)).abs()
            worst = max(worst, int(ulps.max()))
            assert ulps.max() <= 2, (spec, int(ulps.max()), int(ulps.argmax()))
            if name == "ties":  # g = ||v||: the packers' scale is exactly 1 and the stream holds the snapped v itself
                v = sd[spec[1] + ".weight_v"].double()
                assert torch.equal(got.view(torch.int32), _expected_f32(v, bias, slots, nb)[0].float().view(torch.int32)), spec
        else:
            assert torch.equal(got.view(torch.int32), want.view(torch.int32)), (spec, int((got.view(torch.int32) != want.view(torch.int32)).sum()))
        assert torch.equal(got.view(torch.int32)[~used], torch.zeros(int((~used).sum()), dtype=torch.int32)), spec
    print(f"{name}: weight-norm layers within {worst} ulp of the fp64 fold, every other word equal")


def _b_words(sd, l, spec, n_out, slots, nb, f32_layer):
    """The bf16x3 stream of layer l (un-hoisted), uint32 [S][nb][2 parts][64 lanes][4]: element j = 2 i + half of word i of lane (r, h) at step s
    is k-pair 8 s + j, i.e. the fp32 stream's word [t = 8 s + j][lane][ob] -- taken from the CHECKED fp32 layer `f32_layer`, so that the value
    whose parts are expected is the packer's own folded fp32 number at the position the fp32 stream proves.  Returns (hi, lo) (S, nb, 64, 8)."""
    T = slots.numel() // 2
    S = (T + 7) // 8
    v = torch.zeros(S * 8, 64, nb)
    v[:T] = f32_layer.view(T, 64, nb)
    v = v.view(S, 8, 64, nb).permute(0, 3, 2, 1).contiguous()  # (S, nb, lane, j)
    return _bf16_parts(v)


@pytest.mark.parametrize("name", FAMILIES)
def test_bf16x3_streams_hold_the_rounded_parts(name):
    """Streams 1 (bf16x3) and 3 (hoisted bf16x3): each hi word paired with the lo word 1 KB behind it.  hi = torch.bfloat16 round-to-nearest-even
    of the folded fp32 value, lo = the same of value - hi, at every position of stream 1; stream 3 equals stream 1 layer for layer except the
    three hoisted layers, whose (hi, lo) pairs are, as a multiset, those of the layer's per-sample columns.  And |value - hi - lo| <=
    max(2^-16 |value|, 2^-134): two 8-bit significands, down to half a bf16 subnormal step -- derived, not measured.  'ties' pins the tie rule
    and the carry, 'wide' the subnormal low parts, 'sparse' the signed zeros."""
    from vanerf_amd import renderer as R
    sd = _family(name)["sd"]
    f32 = R.stream_host(sd, 0).view(torch.float32)
    s1, s3 = R.stream_host(sd, 1), R.stream_host(sd, 3)
    tabs = _layer_tables()
    hoisted_T = {0: 34, 2: 34, 16: 20}  # layer_spec.h kT_b: [pix32 | 2 scalar pairs], [query6 | latent12 | 2 visibility pairs]
    cols = {0: list(range(64)) + list(range(192, 196)), 2: list(range(64)) + list(range(192, 196)), 16: list(range(11)) + list(range(69, 96))}
    at0 = at1 = at3 = 0
    for l, (spec, n_out, slots) in enumerate(tabs):
        T = slots.numel() // 2
        nb = (n_out + 31) // 32
        n0, S = T * 64 * nb, (T + 7) // 8
        hi, lo = _b_words(sd, l, spec, n_out, slots, nb, f32[at0:at0 + n0])
        words = s1[at1:at1 + S * nb * 512].view(S, nb, 2, 64, 4).long()
        got = torch.stack([words & 0xffff, (words >> 16) & 0xffff], -1).reshape(S, nb, 2, 64, 8)
        assert torch.equal(got[:, :, 0], hi), (spec, "hi", int((got[:, :, 0] != hi).sum()))
        assert torch.equal(got[:, :, 1], lo), (spec, "lo", int((got[:, :, 1] != lo).sum()))
        # the derived bound on what the two parts leave
        T8 = torch.zeros(S * 8, 64, nb)
        T8[:T] = f32[at0:at0 + n0].view(T, 64, nb)
        v = T8.view(S, 8, 64, nb).permute(0, 3, 2, 1).double()
        back = lambda p: (p << 16).to(torch.int32).view(torch.float32).double()
        rest = (v - back(got[:, :, 0]) - back(got[:, :, 1])).abs()
        assert (rest <= torch.clamp(2.0 ** -16 * v.abs(), min=2.0 ** -134)).all(), spec
        Sh = (hoisted_T.get(l, T) + 7) // 8
        chunk3 = s3[at3:at3 + Sh * nb * 512]
        if l not in hoisted_T:
            assert torch.equal(chunk3, s1[at1:at1 + S * nb * 512]), spec
        else:
            w3 = chunk3.view(Sh, nb, 2, 64, 4).long()
            g3 = torch.stack([w3 & 0xffff, (w3 >> 16) & 0xffff], -1).reshape(Sh, nb, 2, 64, 8)
            pairs = (g3[:, :, 0] << 16 | g3[:, :, 1]).reshape(-1)
            W = _layer_folded(sd, spec, n_out)[0].float()[:, cols[l]]
            whi, wlo = _bf16_parts(W.reshape(-1))
            want = whi << 16 | wlo
            zero = lambda p: (p & 0x7fff7fff) == 0  # +-0 | +-0: a zero weight is indistinguishable from padding
            assert torch.equal(torch.sort(pairs[~zero(pairs)])[0], torch.sort(want[~zero(want)])[0]), spec
        at0, at1, at3 = at0 + n0, at1 + S * nb * 512, at3 + Sh * nb * 512
    assert at0 + 512 == f32.numel() and at1 + 512 == s1.numel() and at3 + 512 == s3.numel()


def test_host_packer_keeps_a_nan_with_a_full_payload():
    """bf16 rounding adds 0x7fff to the raw bits: a NaN whose significand is all ones (0x7fffffff) would carry over into the sign and come
    out as -0.0 in both parts -- a diverged checkpoint would render finite images from a bf16x3 handle.  Both parts must stay NaN."""
    from vanerf_amd import renderer as R
    sd = synth.make_full_weights(0)
    key = "mlp_geo.layers1.layers.3.linear.weight"
    base = R.stream_host(sd, 1)
    w = sd[key].clone()
    w.view(torch.int32)[5, 7] = 0x7fffffff
    s = R.stream_host(dict(sd, **{key: w}), 1)
    changed = (s != base).nonzero().view(-1)
    assert changed.numel() == 2 and changed[1] - changed[0] == 256  # the hi word and the lo word 1 KB behind it
    for i in changed:
        halves = {(int(s[i]) & 0xffff), (int(s[i]) >> 16) & 0xffff} - {(int(base[i]) & 0xffff), (int(base[i]) >> 16) & 0xffff}
        assert halves == {0x7fc0}, [hex(h) for h in halves]


# ---------------------------------------------------------------------------------------------------------------------
# 3. on the device
# ---------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def R():
    if not torch.cuda.is_available():
        pytest.fail("GPU tests need a GPU (torch.cuda.is_available() is False)")
    from vanerf_amd import renderer
    return renderer


_GPU = {}


def _case(R, name):
    """_family(name) plus the device side, built once: FrameData, the device's 1-NN, the fp64 outputs with the DEVICE's vert_vis, E32 and A."""
    from tests.test_hip_parity import _frame_data, dev
    if name not in _GPU:
        c = dict(_family(name))
        sd, frame, pts = c["sd"], c["frame"], c["pts"]
        c["fdat"] = _frame_data(R, sd, frame)
        c["knn"] = R.knn1(c["fdat"].verts4, dev(pts))
        vv = c["fdat"].vert_vis.cpu()
        assert torch.equal(vv, c["vert_vis"])
        sd64 = cast(sd, torch.float64)
        c["want"] = orc.eval_func(sd64, c["r64"]["raw"][None], c["r64"]["valid"][None, :, None], 100.0)[0]
        want32 = orc.eval_func(sd, c["r32"]["raw"][None], c["r32"]["valid"][None, :, None], 100.0)[0]
        c["E32"] = (want32.double() - c["want"]).abs().max(0)[0]
        c["A"] = max(y.abs().max().item() for _, y in c["r64"]["layers"].values())
        _GPU[name] = c
    return _GPU[name]


def _bars(c, kernel):
    """gains: per-output bar from the oracle alone (module docstring)."""
    bar = 4.0 * c["E32"] + (2.0 ** -15 * c["A"] if kernel != "fp32" else 0.0)
    return torch.clamp(bar, min=TOL)


@pytest.mark.gpu
@pytest.mark.parametrize("precision", ["fp32", "bf16x3"])
@pytest.mark.parametrize("name", FAMILIES)
def test_device_packer_equals_the_host_packer_on_every_family(R, name, precision):
    """A handle packed from the recipe and re-packed in place from the family on the device (vanerf_weights_update) holds the bits of the
    host packer's streams of the family: forward, backward (fp32 handles), hoisted (bf16x3 handles), the clamped sigmoid_beta; and the other
    way round, family -> recipe, where a word left over from the family (a value where a zero belongs, a zero where a value belongs) would
    show.  Fold and bf16 split run as separate code on the two sides; test_fp32_stream... / test_bf16x3_streams... pin the host side."""
    which = {"fp32": 0, "bf16x3": 1}[precision]
    hot, fam = synth.make_full_weights(0), _family(name)["sd"]
    for first, second in ((hot, fam), (fam, hot)):
        w = R.PackedWeights(first, mode=precision)
        assert torch.equal(R.stream_device(w, 0), R.stream_host(first, which))
        w.update({k: v.cuda() for k, v in second.items()})
        assert torch.equal(R.stream_device(w, 0), R.stream_host(second, which))
        if precision == "fp32":
            assert torch.equal(R.stream_device(w, 2), R.stream_host(second, 2))
        else:
            assert torch.equal(R.stream_device(w, 3), R.stream_host(second, 3))
        assert w.beta == max(second["sigmoid_beta"].item(), 2e-3)
    if name == "gains":
        w.update({k: v.cuda() for k, v in synth.make_weight_family("gains", 2).items()})
        assert w.beta == 2e-3  # 1e-3 lies below the clamp


@pytest.mark.gpu
@pytest.mark.parametrize("kernel", ["fp32", "bf16x3", "bf16x3_hoisted"])
@pytest.mark.parametrize("name", FAMILIES)
def test_forward_kernels_on_every_family(R, name, kernel):
    """vanerf_query_samples (fp32, bf16x3) and its hoisted form with vertex_products on N_POINTS points of pose A against the fp64 oracle: equal
    validity flags and 1-NN indices; wide / ties / sparse within 1e-4 and the sigma check of tests/test_posed_source.py; gains within the bar
    computed from the oracle alone, sigma with each sigmoid_beta of the family as the handle clamps it."""
    from tests.test_posed_source import _run_kernel, _within_the_bar
    c = _case(R, name)
    got, valid = _run_kernel(R, c["sd"], c, kernel)
    assert torch.equal(c["knn"].cpu().long(), orc.knn1(c["pts"], c["frame"]["targets"]["vert_world"][0]))
    assert torch.equal(valid, c["r64"]["valid"]), f"{int((valid != c['r64']['valid']).sum())} validity flags differ"
    err = (got.double() - c["want"]).abs().max(0)[0]
    print(f"{name} [{kernel}]: E32 {[f'{e:.2e}' for e in c['E32'].tolist()]}, A {c['A']:.3e}, max |HIP - fp64| {[f'{e:.2e}' for e in err.tolist()]}")
    if name != "gains":
        _within_the_bar(got, c["want"], f"{name} [{kernel}]")
        return
    bar = _bars(c, kernel)
    print(f"{name} [{kernel}]: bar {[f'{b:.2e}' for b in bar.tolist()]}")
    assert torch.isfinite(got).all()
    for b in synth.GAINS_BETAS:
        beta = R.PackedWeights(dict(c["sd"], sigmoid_beta=torch.tensor([b])), mode=kernel.split("_")[0]).beta
        assert beta == max(torch.tensor(b).item(), 2e-3)
        _within_the_bar(got, c["want"], f"{name} [{kernel}] beta {beta:g}", beta=beta, tol=bar, sigma_tol=bar[0].item() / (4.0 * beta))


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["sparse", "ties"])
def test_hoisted_equals_unhoisted_on_zeros_and_ties(R, name):
    """The per-vertex products (fp32 fmaf chains over hi + lo, vertex_products.hip) take the place of MFMA k-steps: on zero columns / rows and
    on tie values both bf16x3 variants give the same validity flags and stay within 1e-4 of each other and of the fp32 kernel, as
    tests/test_vertex_products.py allows; on 'sparse' an all-zero output row gives the same (exactly zero) contribution either way."""
    from tests.test_posed_source import _run_kernel
    c = _case(R, name)
    ref, valid = _run_kernel(R, c["sd"], c, "fp32")
    plain, valid_p = _run_kernel(R, c["sd"], c, "bf16x3")
    hoisted, valid_h = _run_kernel(R, c["sd"], c, "bf16x3_hoisted")
    assert torch.equal(valid_p, valid) and torch.equal(valid_h, valid)
    d_var, d_ref, d_p = (hoisted - plain).abs().max().item(), (hoisted - ref).abs().max().item(), (plain - ref).abs().max().item()
    print(f"{name}: hoisted vs un-hoisted bf16x3 {d_var:.3e}, hoisted vs fp32 {d_ref:.3e}, un-hoisted vs fp32 {d_p:.3e}")
    assert d_var <= TOL and d_ref <= TOL and d_p <= TOL


@pytest.mark.gpu
@pytest.mark.parametrize("precision", ["fp32", "bf16x3"])
@pytest.mark.parametrize("beta", [0.02, 1e-3])
def test_composite_with_the_familys_sigmoid_beta(R, beta, precision):
    """One render_pass of 16 x 16 rays, 16 + 16 samples with the oracle's rays injected, on 'gains' with sigmoid_beta 0.02 and 1e-3 (clamped
    to 2e-3: sigma reaches 500), against the oracle's networks and composite in fp64 at the same sample positions.  Bar per image, from the
    oracle alone as for the forward kernels: max(1e-4, 4 E32 [+ 2^-15 A for bf16x3]), E32 = |fp32 oracle - fp64 oracle| of that image.

    Over all pixels that bar is loose at the clamp: on a nearly empty ray the fp32 oracle's depth is 0.46 off the fp64 oracle's (below).
    So the same bar is applied a second time to the CLEAN pixels alone, with E32 taken over them: sigma is a step of height 500, and a sample
    is at risk when it is valid and |rad| <= m + 40 beta + |q_sdf|, m = the forward kernel's bar on alpha (4 max |rad32 - rad64|
    [+ 2^-15 A]).  Below -m alpha is exactly 0 on every side; above m + 40 beta + |q_sdf| the sigmoid's argument exceeds 40 on every side and
    sigma is 0 to 1e-15: on a pixel without a sample at risk sigma is the same function of q_sdf everywhere and only the colour and sdf
    outputs' own errors reach the images.  And depth and sdf are sums over contrib divided by acc + 1e-8: on a nearly empty ray (acc of the
    order of 1e-8) fp32 loses a contribution to 1 - exp(-x), x < 6e-8, and the ratio moves by O(1), so a clean pixel also has acc > 0.05
    (S 6e-8 / acc is then below 1e-4) or acc < 1e-13 (both sides give 0), acc the fp64 oracle's.  More than half of the pixels must be clean."""
    from tests.test_hip_injected import COARSE, FINE, _inject
    from tests.test_hip_parity import _frame_data
    from tests.test_posed_source import _images_fp64
    key = ("pass", beta)
    if key not in _GPU:
        sd = synth.make_weight_family("gains", 0, sigmoid_beta=beta)
        frame = posed_frame("A", 3)
        ref = orc.batch_render(sd, frame, 3, torch.tensor([[[1, 2]]]), 16, 16)
        ref64 = _images_fp64(sd, frame, ref)
        A, parts = 0.0, []
        for part in (ref["coarse"], ref["fine"]):
            args = (sd, frame, part["pts"][0], part["q_sdf"].reshape(-1), part["q_vis"].reshape(-1), part["vert_vis"].reshape(-1))
            r, r32 = reference(*args), reference(*args, dtype=torch.float32)
            A = max(A, max(y.abs().max().item() for _, y in r["layers"].values()))
            assert torch.equal(r["valid"], r32["valid"])
            e_rad = (r32["raw"][:, 1].double() - r["raw"][:, 1])[r["valid"]].abs().max().item()
            parts.append((r["raw"][:, 1].view(256, -1), r["valid"].view(256, -1), part["q_sdf"].double().view(256, -1), e_rad))
        _GPU[key] = (sd, frame, ref, ref64, A, parts, _frame_data(R, sd, frame))
    sd, frame, ref, ref64, A, parts, fdat = _GPU[key]
    assert all(torch.isfinite(v).all() for v in ref64.values())
    w = R.PackedWeights(sd, mode=precision)
    assert w.beta == max(torch.tensor(beta).item(), 2e-3)
    out = R.render_pass(w, fdat, frame["cam_tar"], frame["bounds"], 1, 2, 4, 16, 16, 16, 16, inject=_inject(ref))
    assert torch.equal(out["index"].cpu(), ref["index"][0])
    lo_lo = 2.0 ** -15 * A if precision == "bf16x3" else 0.0
    clean = []
    for (rad, valid, q_sdf, e_rad), acc in zip(parts, (ref64["alpha"][0], ref64["alpha_fine"][0])):
        at_risk = valid & (rad.abs() <= 4.0 * e_rad + lo_lo + 40.0 * w.beta + q_sdf.abs())
        clean.append(~at_risk.any(1).view(16, 16) & ((acc > 0.05) | (acc < 1e-13)))
        assert clean[-1].float().mean() > 0.5, clean[-1].float().mean().item()
    bad = []
    for k, gk, ch in COARSE + FINE:
        got = out[k].cpu().view(16, 16, 3).permute(2, 0, 1) if ch == 3 else out[k].cpu().view(16, 16)
        pix = clean[0 if (k, gk, ch) in COARSE else 1]
        e32_all, err_all = (ref[gk][0].double() - ref64[gk][0]).abs(), (got.double() - ref64[gk][0]).abs()
        for what, e32, err in (("all pixels", e32_all.max().item(), err_all.max().item()),
                               (f"{int(pix.sum())} clean pixels", e32_all[..., pix].max().item(), err_all[..., pix].max().item())):
            bar = max(TOL, 4.0 * e32 + lo_lo)
            print(f"gains beta {w.beta:g} [{precision}] {gk}, {what}: E32 {e32:.2e}, A {A:.3e}, bar {bar:.2e}, max |HIP - fp64| {err:.2e}")
            if not err <= bar:
                bad.append((gk, what, err, bar))
    assert not bad, bad
    assert ref64["depth_fine"].std() > 1e-3 and 0.05 < ref["coarse"]["rgba"][..., 0].gt(0).float().mean() < 0.95


@pytest.mark.gpu
@pytest.mark.parametrize("name,variant", [("sparse", "d_noise"), ("gains", "d_d2_noise")])
def test_fused_backward_on_sparse_and_gains(R, name, variant):
    """vanerf_query_forward_spill + vanerf_query_backward + vanerf_weight_products on 600 points of pose A against fp64 autograd with the
    helper and the relative bounds of tests/test_backward_per_sample.py; and wherever fp64 autograd gives an exactly zero parameter gradient
    (a zero output row in front of a ReLU passes nothing back; an operand that is zero on every sample) the kernels give exactly zero."""
    from tests.test_backward_per_sample import check_block_against_fp64
    from vanerf_amd import hip_backward as HB
    c = _case(R, name)
    env = (HB, R, c["sd"], c["frame"], c["fdat"], R.PackedWeights(c["sd"], mode="fp32"))
    pts = near_mesh_points(c["frame"], 600, seed=4)
    assert decision_margins(c["frame"], pts)[0].min() > 1e-5
    valid, knn, q_vis, flip, worst = check_block_against_fp64(env, pts, variant, zeros_exact=True)
    assert 0.05 < valid.float().mean() < 0.95 and bool(q_vis.any()) and not bool(q_vis.all())
    if name == "sparse":
        assert worst["exact zeros"] > 1000  # whole rows and columns of parameter gradients, beyond fconv.2's unused rows


@pytest.mark.gpu
@pytest.mark.parametrize("precision", ["fp32", "bf16x3"])
@pytest.mark.parametrize("bad", ["nan", "inf"])
def test_non_finite_weights_give_non_finite_outputs(R, bad, precision):
    """One NaN (payload 0x7fffffff, the one bf16 rounding by bit arithmetic wraps into -0.0) or one +inf in mlp_geo.layers1's last matrix,
    which every valid sample passes through: a plain launch on bad numbers.  On every valid sample sdf is non-finite in every kernel of
    the mode and alpha is exactly 0 (NaN) / 0 or non-finite (+inf); the device packer holds the host packer's bits of the bad element.  (The kernels'
    ReLU is max(x, 0) in one instruction, which returns 0 for a NaN where torch.relu returns NaN: alpha of a NaN rad is 0 and the colour
    behind TexVisFusion's ReLUs is 0, in both modes alike -- DESIGN.md section 5b.  The sdf output has no ReLU behind the bad element.)"""
    from tests.test_posed_source import KERNELS, _run_kernel
    c = _case(R, "wide")
    key = "mlp_geo.layers1.layers.3.linear.weight"
    w = c["sd"][key].clone()
    w.view(torch.int32)[5, 7] = 0x7fffffff if bad == "nan" else 0x7f800000
    sd = dict(c["sd"], **{key: w})
    which = {"fp32": 0, "bf16x3": 1}[precision]
    h = R.PackedWeights(c["sd"], mode=precision).update({k: v.cuda() for k, v in sd.items()})
    assert torch.equal(R.stream_device(h, 0), R.stream_host(sd, which))
    if precision == "bf16x3":
        assert torch.equal(R.stream_device(h, 3), R.stream_host(sd, 3))
    for kernel in [k for k, (mode, _) in KERNELS.items() if mode == precision]:
        got, valid = _run_kernel(R, sd, c, kernel)
        assert torch.equal(valid, c["r64"]["valid"]) and valid.any()
        v = got[valid]
        assert not torch.isfinite(v[:, 1]).any(), (kernel, int(torch.isfinite(v[:, 1]).sum()))
        # alpha: pinned at the kernels' present max(NaN, 0) = 0 (torch.relu gives NaN), so that a NaN-preserving ReLU changes this
        # line knowingly; behind +inf the pooled variance is inf - inf = NaN as well, or rad itself is +inf
        if bad == "nan":
            assert torch.equal(v[:, 0], torch.zeros_like(v[:, 0])), (kernel, int((v[:, 0] != 0).sum()))
        else:
            assert ((v[:, 0] == 0) | ~torch.isfinite(v[:, 0])).all(), kernel


# ---------------------------------------------------------------------------------------------------------------------
# 4. VANeRF follows a change of `precision`
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_packed_weights_follow_a_change_of_precision(R):
    """net.precision flipped between passes: packed_weights() and packed_weights('fp32') return handles of the requested mode whose streams
    are the host packer's for that mode (a held handle of the other mode is re-packed in place by vanerf_weights_update, which keeps its
    mode: it must not be re-used), and a training step after the flip runs -- the fused backward refuses a bf16x3 handle."""
    from tests.test_autograd import _net, _step
    net = _net(0.01)
    frame = synth.to_device(synth.make_frame(seed=3, tar_h=64, tar_w=64), "cuda")
    opt = torch.optim.Adam(net.parameters(), lr=1e-3)
    assert net.precision == "bf16x3"

    def check():
        sd = {k: v.detach().cpu() for k, v in net._hot_state().items()}
        own, w0 = net.packed_weights(), net.packed_weights("fp32")
        assert own.mode == R.PRECISIONS[net.precision] and w0.mode == 0
        assert torch.equal(R.stream_device(own, 0), R.stream_host(sd, own.mode))
        assert torch.equal(R.stream_device(w0, 0), R.stream_host(sd, 0)) and torch.equal(R.stream_device(w0, 2), R.stream_host(sd, 2))
        if own.mode:
            assert torch.equal(R.stream_device(own, 3), R.stream_host(sd, 3))

    for precision in ("bf16x3", "fp32", "bf16x3", "fp32"):
        net.precision = precision
        out = _step(net, frame)
        check()
        opt.zero_grad(set_to_none=True)
        ((out["tex_fg_fine"] - out["tar_img"]).abs().mean() + out["alpha_fine"].mean()).backward()
        assert all(torch.isfinite(p.grad).all() for p in net.parameters() if p.grad is not None)
        opt.step()  # the parameters change: the next packed_weights() takes the re-pack path with a held handle of the other mode
        check()
