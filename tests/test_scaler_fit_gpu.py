"""Scaler fitting on the GPU (csrc/scaler_fit.hip, DeviceBatchScaler.fit): the radix select against torch.sort of the CPU
copy (equal as numbers), the fit against the live reference's (tests/golden/scaler_fit.npz: MEG tables, category counts
and weights EQUAL; StandardScaler values within one fp32 ulp of the fp64 statistic; the transform round trip EQUAL
wherever the tables are, and in every channel once the reference's own StandardScaler values sit in the tables), the
category counter, the inverse transform bit for bit, and non-finite values."""
import numpy as np
import pytest
import torch

from helpers import Golden
from test_scaler_fit_cpu import CASES, FitBatch, fixture_loaders

pytestmark = pytest.mark.gpu
DEV = "cuda"

SHAPES = [(1, 1, 1), (3, 5, 7), (9, 3, 40), "misaligned", (40, 4, 360), (200, 2, 360)]
DATA = ["gaussian", "negative", "ties", "constant_column", "low_byte", "top_byte", "special"]


def from_bits(bits: torch.Tensor) -> torch.Tensor:
    return torch.from_numpy(bits.numpy().astype(np.uint32).view(np.float32).copy())


def make_data(kind: str, shape, gen) -> torch.Tensor:
    if kind == "gaussian":
        return torch.randn(shape, generator=gen)
    if kind == "negative":
        return -torch.randn(shape, generator=gen).abs() - 0.1
    if kind == "ties":
        return torch.randint(-3, 4, shape, generator=gen).float()
    if kind == "constant_column":
        x = torch.randn(shape, generator=gen)
        x[:, 0] = 2.5
        return x
    if kind == "low_byte":                     # keys that differ only in the lowest byte
        return 1.0 + torch.randint(0, 256, shape, generator=gen).float() * 2.0 ** -23
    if kind == "top_byte":                     # keys that differ only in the top byte (all finite: bit 23 is clear)
        return from_bits((torch.randint(0, 256, shape, generator=gen) << 24) | 0x123456)
    assert kind == "special"                   # denormals, +-0.0, +-inf among ordinary values
    x = torch.randn(shape, generator=gen)
    pick = torch.randint(0, 8, shape, generator=gen)
    sign = torch.randint(0, 2, shape, generator=gen) << 31
    x = torch.where(pick == 0, from_bits(torch.randint(1, 1000, shape, generator=gen) | sign), x)
    x = torch.where(pick == 1, from_bits(sign), x)
    x = torch.where(pick == 2, from_bits(0x7f800000 | sign), x)
    return x


def on_device(x: torch.Tensor, misaligned: bool = False) -> torch.Tensor:
    if not misaligned:
        return x.to(DEV)
    base = torch.empty(x.numel() + 1, device=DEV)
    view = base[1:].view(x.shape)              # contiguous, 4 bytes off the allocation's 16-byte alignment
    view.copy_(x)
    assert view.is_contiguous() and view.data_ptr() % 16 == 4
    return view


def sorted_columns(x: torch.Tensor) -> torch.Tensor:
    """[C, n]: every column x[:, c, :] of the CPU tensor sorted ascending by torch.sort (NaNs last)."""
    return x.permute(1, 0, 2).reshape(x.shape[1], -1).sort(dim=1).values


def rank_sets(n: int):
    quant = [int(q * n) for q in (0.25, 0.5, 0.75)]
    eight = sorted([0, n // 7, n // 7, n // 3, n // 2, n // 2, n - 1, n - 1])
    return [[0, n - 1], quant, eight]


def same_numbers(got: torch.Tensor, want: torch.Tensor) -> bool:
    """Equal as numbers (-0.0 == +0.0), NaN where and only where the other has NaN."""
    nan = want.isnan()
    return torch.equal(got.isnan(), nan) and torch.equal(got.masked_fill(nan, 0), want.masked_fill(nan, 0))


@pytest.mark.parametrize("kind", DATA)
@pytest.mark.parametrize("shape", SHAPES, ids=str)
def test_quantile_select_equals_torch_sort(shape, kind):
    from brainmagick_amd import hip_ops as H
    misaligned = shape == "misaligned"
    shape = (9, 3, 40) if misaligned else shape
    gen = torch.Generator().manual_seed(11 + sum(shape) + DATA.index(kind))
    x = make_data(kind, shape, gen)
    cols = sorted_columns(x)
    xd = on_device(x, misaligned)
    for ranks in rank_sets(shape[0] * shape[2]):
        got = H.quantile_select(xd, ranks).cpu()
        assert got.shape == (shape[1], len(ranks))
        assert torch.equal(got, cols[:, ranks]), (shape, kind, ranks)


@pytest.mark.parametrize("shape", [(9, 3, 40), (200, 2, 360)], ids=str)
def test_quantile_select_puts_every_nan_last(shape):
    """torch.sort puts all NaNs last whatever their sign bit: the ranks below the NaN block are exact, those inside it
    return NaN; an all-NaN column returns NaN."""
    from brainmagick_amd import hip_ops as H
    gen = torch.Generator().manual_seed(5)
    x = torch.randn(shape, generator=gen)
    u = torch.rand(shape, generator=gen)
    x = torch.where(u < 0.05, from_bits(torch.full(shape, 0x7fc00000)), x)
    x = torch.where((u >= 0.05) & (u < 0.10), from_bits(torch.full(shape, 0xffc00001)), x)
    x[:, -1] = from_bits(torch.full((shape[0], shape[2]), 0xffc00000))        # an all-NaN column
    n = shape[0] * shape[2]
    n_nan = int(x[:, 0].isnan().sum())
    assert 0 < n_nan < n // 4
    cols = sorted_columns(x)
    ranks = [0, n // 2, n - n_nan - 1, n - n_nan, n - 1]
    got = H.quantile_select(x.to(DEV), ranks).cpu()
    assert same_numbers(got, cols[:, ranks])
    assert not got[0, :3].isnan().any() and got[0, 3:].isnan().all() and got[-1].isnan().all()


def test_quantile_select_is_deterministic_and_checks_its_arguments():
    from brainmagick_amd import hip_ops as H
    x = torch.randn(200, 2, 360, generator=torch.Generator().manual_seed(9)).to(DEV)
    ranks = [int(q * 72000) for q in (0.25, 0.5, 0.75)]
    a, b = H.quantile_select(x, ranks), H.quantile_select(x, ranks)
    assert torch.equal(a.view(torch.int32), b.view(torch.int32))
    with pytest.raises(RuntimeError):
        H.quantile_select(x, [5, 3])                       # not ascending
    with pytest.raises(RuntimeError):
        H.quantile_select(x, [72000])                      # outside [0, n)
    with pytest.raises(RuntimeError):
        H.quantile_select(x, list(range(9)))               # more than 8 ranks
    with pytest.raises(RuntimeError):
        H.quantile_select(x.cpu(), ranks)
    assert H.quantile_select(x[:0], [0]).shape == (2, 1)   # empty input: nothing to do


# ---- DeviceBatchScaler.fit against the live reference ----------------------------------------------------------------
class Builder:
    """The surface of bm.features.FeaturesBuilder that fitting touches."""

    def __init__(self, spec):
        self.features, self.slices, start = {}, {}, 0
        for name, dim, kind, cardinality in spec:
            self.features[name] = type("Feature", (), dict(normalizable=kind == "normalizable",
                                                           categorical=kind == "categorical",
                                                           cardinality=cardinality))()
            self.slices[name] = slice(start, start + dim)
            start += dim
        self.dimension = start

    def items(self):
        return self.features.items()

    def get_slice(self, name):
        return self.slices[name]


_fitted = {}


def fitted(case):
    """(fixture, scaler fitted on the fixture's inputs), once per case."""
    from brainmagick_amd.norm import DeviceBatchScaler
    if case not in _fitted:
        g = Golden("scaler_fit")
        kw = g.meta["cases"][case]["kwargs"]
        scaler = DeviceBatchScaler.fit(fixture_loaders(g, DEV), Builder(g.meta["features"]),
                                       n_samples_per_recording=g.meta["dims"]["n_samples_per_recording"], **kw)
        _fitted[case] = (g, scaler)
    return _fitted[case]


def roundtrip_batch(g):
    return FitBatch(g.t("roundtrip_in/meg").to(DEV), g.t("roundtrip_in/features").to(DEV),
                    g.t("roundtrip_in/mask").to(DEV), g.t("roundtrip_in/recording_index").to(DEV))


def ulp32(v) -> np.ndarray:
    return np.spacing(np.abs(np.asarray(v, dtype=np.float64)).astype(np.float32)).astype(np.float64)


@pytest.mark.parametrize("case", CASES)
def test_fit_equals_the_reference(case):
    from brainmagick_amd.norm import DeviceBatchScaler
    g, scaler = fitted(case)
    for rec in (0, 1, 2):
        assert torch.equal(scaler.meg_center[rec].cpu(), g.t(f"{case}/meg_center/{rec}")), rec
        assert torch.equal(scaler.meg_scale[rec].cpu(), g.t(f"{case}/meg_scale/{rec}")), rec
    assert (g.t(f"{case}/meg_scale/2")[4] == 1).all()                          # the constant sensor
    assert torch.equal(scaler.categories_count["cat"], g.t(f"{case}/cat_count"))
    assert scaler.categories_count["cat"][3] == 0
    assert torch.equal(scaler.get_categorical_feature_weights("cat"), g.t(f"{case}/cat_weights"))
    # the no-op and categorical channels are left alone
    assert torch.equal(scaler.feature_center[4:].cpu(), torch.zeros(2))
    assert torch.equal(scaler.feature_scale[4:].cpu(), torch.ones(2))
    # inverse_transform(transform(batch)): equal wherever the tables are equal -- the MEG and the untouched feature channels
    want = g.t(f"{case}/roundtrip/features")
    back = scaler.inverse_transform(scaler.transform(roundtrip_batch(g)))
    assert torch.equal(back.meg.cpu(), g.t(f"{case}/roundtrip/meg"))
    assert torch.equal(back.features[:, 4:].cpu(), want[:, 4:])
    # ... and, with the reference's own fp32 StandardScaler values in the tables, in every feature channel: the two
    # kernels reproduce the reference's arithmetic bit for bit
    ref_tables = DeviceBatchScaler(scaler.meg_center, scaler.meg_scale,
                                   torch.cat([g.t(f"{case}/emb_center").expand(4), torch.zeros(2)]),
                                   torch.cat([g.t(f"{case}/emb_scale").expand(4), torch.ones(2)]))
    ref_tables.feature_slices, ref_tables.feature_kinds = scaler.feature_slices, scaler.feature_kinds
    back_ref = ref_tables.inverse_transform(ref_tables.transform(roundtrip_batch(g)))
    assert torch.equal(back_ref.meg.cpu(), g.t(f"{case}/roundtrip/meg"))
    assert torch.equal(back_ref.features.cpu(), want)
    one = ref_tables.inverse_transform_feature("emb", ref_tables.transform(roundtrip_batch(g)).features[:, :4])
    assert torch.equal(one.cpu(), want[:, :4])
    aux = back_ref.features[:, 5:]
    assert ref_tables.inverse_transform_feature("aux", aux) is aux            # a no-op scaler returns its input
    # The fitted StandardScaler values are the rounded fp64 statistic, up to one ulp off the reference's fp32 sums
    # (test_fit_standard_scaler_is_the_rounded_fp64_statistic), so the normalizable channels come back as x up to
    # the four roundings of ((x - c) / s) * s + c: at most 1/2 ulp each at magnitudes <= |x| + |c| (twice that for the
    # quotient's, which is scaled by s across a binade): 5/2 ulp(|x| + |c|) for either side of the comparison.
    x = g.t("roundtrip_in/features")[:, :4].double().numpy()
    c = np.abs(scaler.feature_center[:4].cpu().double().numpy())[None, :, None]
    bound = 2.5 * ulp32(np.abs(x) + c)
    ours = back.features[:, :4].cpu().double().numpy()
    print(case, "emb round trip: max |ours - x| / ulp", (np.abs(ours - x) / ulp32(np.abs(x) + c)).max(),
          "max |ours - reference| / ulp", (np.abs(ours - want[:, :4].double().numpy()) / ulp32(np.abs(x) + c)).max())
    assert (np.abs(ours - x) <= bound).all()
    assert (np.abs(ours - want[:, :4].double().numpy()) <= 2 * bound).all()


@pytest.mark.parametrize("case", CASES)
def test_fit_standard_scaler_is_the_rounded_fp64_statistic(case):
    """The reference sums in fp32; ours is the fp32 rounding of an fp64 sum: within one fp32 ulp of the fp64 statistic,
    and no further from the reference's number than the reference's own deviation plus one ulp."""
    g, scaler = fitted(case)
    for ours, key in ((scaler.feature_center, "emb_center"), (scaler.feature_scale, "emb_scale")):
        ours = ours[:4].cpu().double().numpy()
        exact = np.broadcast_to(g.raw[f"{case}/{key}_f64"], (4,))
        ref = np.broadcast_to(g.raw[f"{case}/{key}"].astype(np.float64), (4,))
        print(case, key, "ours - fp64", ours - exact, "reference - fp64", ref - exact, "ulp", ulp32(exact))
        assert (np.abs(ours - exact) <= ulp32(exact)).all()
        assert (np.abs(ours - ref) <= np.abs(ref - exact) + ulp32(exact)).all()


def test_fitted_scaler_drives_scale_reject_like_the_reference_tables():
    from brainmagick_amd.norm import DeviceBatchScaler, ScaleReject
    g, scaler = fitted("default")
    center = torch.stack([g.t(f"default/meg_center/{r}") for r in range(3)])
    scale = torch.stack([g.t(f"default/meg_scale/{r}") for r in range(3)])
    fcenter = torch.cat([g.t("default/emb_center").expand(4), torch.zeros(2)])
    fscale = torch.cat([g.t("default/emb_scale").expand(4), torch.ones(2)])
    tables = DeviceBatchScaler(center, scale, fcenter, fscale)
    batch = roundtrip_batch(g)
    batch.meg[1] *= 1000.0
    batch.meg[4, 2, 5] = 1e6
    for clip in (False, True):
        a, keep_a = ScaleReject(scaler, limit=16, clip=clip)(batch)
        b, keep_b = ScaleReject(tables, limit=16, clip=clip)(batch)
        assert torch.equal(keep_a, keep_b) and torch.equal(a.meg, b.meg)
        assert keep_a.tolist() == ([True] * 6 if clip else [True, False, True, True, False, True])


def test_fit_without_features_and_with_narrow_recordings():
    """features_builder=None fits the MEG only; a recording with fewer channels than the table is wide keeps
    centre 0 / scale 1 in the tail."""
    from brainmagick_amd.norm import DeviceBatchScaler
    g = Golden("scaler_fit")
    loaders = fixture_loaders(g, DEV)
    loaders[1] = [b.replace(meg=b.meg[:, :4].contiguous()) for b in loaders[1]]          # recording 0: 4 sensors
    scaler = DeviceBatchScaler.fit(loaders, n_samples_per_recording=10)
    assert scaler.feature_center is None and scaler.meg_center.shape == (3, 6)
    assert torch.equal(scaler.meg_center[0].cpu(), torch.cat([g.t("default/meg_center/0")[:4], torch.zeros(2)]))
    assert torch.equal(scaler.meg_scale[0].cpu(), torch.cat([g.t("default/meg_scale/0")[:4], torch.ones(2)]))
    assert torch.equal(scaler.meg_scale[2].cpu(), g.t("default/meg_scale/2"))


def test_fit_nan_reaches_only_its_own_sensor():
    """A sensor of one recording with 60 % NaNs: its median and upper quartile are NaN (torch.sort puts them last), so
    its centre and scale are NaN; every other sensor and recording stays exact."""
    from brainmagick_amd.norm import DeviceBatchScaler
    g = Golden("scaler_fit")
    loaders = fixture_loaders(g, DEV)
    for b in loaders[2]:                                    # recording 1
        b.meg[:, 3, :15] = float("nan")
    scaler = DeviceBatchScaler.fit(loaders, n_samples_per_recording=10)
    center, scale = scaler.meg_center.cpu(), scaler.meg_scale.cpu()
    assert center[1, 3].isnan() and scale[1, 3].isnan()
    center[1, 3] = scale[1, 3] = 0
    want_c, want_s = g.t("default/meg_center/1").clone(), g.t("default/meg_scale/1").clone()
    want_c[3] = want_s[3] = 0
    assert torch.equal(center[1], want_c) and torch.equal(scale[1], want_s)
    for rec in (0, 2):
        assert torch.equal(center[rec], g.t(f"default/meg_center/{rec}"))
        assert torch.equal(scale[rec], g.t(f"default/meg_scale/{rec}"))


# ---- bm_masked_moments ----------------------------------------------------------------------------------------------
def moments_fp64(x, mask, f0, f1, per_channel):
    sel = np.broadcast_to(mask.numpy(), x.shape)[:, f0:f1]
    xs = x.double().numpy()[:, f0:f1]
    if per_channel:
        cols = [xs[:, c][sel[:, c]] for c in range(f1 - f0)]
        return np.array([c.mean() for c in cols]), np.array([c.std(ddof=1) for c in cols])
    picked = xs[sel]
    return np.full(f1 - f0, picked.mean()), np.full(f1 - f0, picked.std(ddof=1))


@pytest.mark.parametrize("per_channel", [False, True])
@pytest.mark.parametrize("shape,full_mask", [((5, 7, 37), False), ((5, 7, 37), True), ((70, 6, 360), False),
                                             ((6, 5, 40), True)])
def test_masked_moments_against_fp64(shape, full_mask, per_channel):
    """Both mask layouts, the dword and the vector path, one and several workgroups per channel; the data has
    mean = 10^3 x std, which an fp32 (or an uncentred) accumulation would not survive."""
    from brainmagick_amd import hip_ops as H
    gen = torch.Generator().manual_seed(21)
    x = 1000.0 + torch.randn(shape, generator=gen)
    N, F, T = shape
    mask = torch.rand((N, F if full_mask else 1, T), generator=gen) > 0.4
    f0, f1 = 1, F - 1
    count, mean, std = H.masked_moments(x.to(DEV), mask.to(DEV), f0, f1, per_channel)
    want_mean, want_std = moments_fp64(x, mask, f0, f1, per_channel)
    sel = np.broadcast_to(mask.numpy(), shape)[:, f0:f1]
    want_count = sel.sum((0, 2)) if per_channel else np.full(f1 - f0, sel.sum())
    assert np.array_equal(count.cpu().numpy(), want_count.astype(np.float64))
    print("mean - fp64", mean.cpu().double().numpy() - want_mean, "std - fp64", std.cpu().double().numpy() - want_std)
    assert (np.abs(mean.cpu().double().numpy() - want_mean) <= ulp32(want_mean)).all()
    assert (np.abs(std.cpu().double().numpy() - want_std) <= ulp32(want_std)).all()
    again = H.masked_moments(x.to(DEV), mask.to(DEV), f0, f1, per_channel)
    assert torch.equal(again[1], mean) and torch.equal(again[2], std)


def test_masked_moments_of_one_and_of_no_value():
    from brainmagick_amd import hip_ops as H
    x = torch.randn(3, 2, 8, generator=torch.Generator().manual_seed(2)).to(DEV)
    mask = torch.zeros(3, 1, 8, dtype=torch.bool, device=DEV)
    count, mean, std = H.masked_moments(x, mask, 0, 2, True)
    assert (count == 0).all() and mean.isnan().all() and std.isnan().all()              # torch: mean / std of nothing
    mask[1, 0, 5] = True
    count, mean, std = H.masked_moments(x, mask, 0, 2, True)
    assert (count == 1).all() and torch.equal(mean, x[1, :, 5]) and std.isnan().all()   # torch.std of one value
    x[0, 0, 0] = float("nan")                                                           # not selected: ignored
    assert torch.equal(H.masked_moments(x, mask, 0, 2, True)[1], x[1, :, 5])


def test_fit_refuses_a_constant_feature():
    """bm/norm.py:233-237: scale > 0 or the fit stops; a constant feature has std exactly 0 here."""
    from brainmagick_amd.norm import DeviceBatchScaler
    gen = torch.Generator().manual_seed(4)
    batch = FitBatch(torch.randn(4, 3, 12, generator=gen).to(DEV), torch.full((4, 2, 12), 0.3, device=DEV),
                     torch.ones(4, 1, 12, dtype=torch.bool, device=DEV), torch.zeros(4, dtype=torch.long, device=DEV))
    with pytest.raises(AssertionError, match="could not be normalized"):
        DeviceBatchScaler.fit([[batch]], Builder([("emb", 2, "normalizable", 0)]))
    with pytest.raises(AssertionError, match="could not be normalized"):      # nothing selected: NaN > 0 is false
        DeviceBatchScaler.fit([[batch.replace(features_mask=~batch.features_mask)]],
                              Builder([("emb", 2, "normalizable", 0)]))


# ---- bm_category_counts ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cardinality,shape", [(2, (3, 2, 7)), (5, (9, 3, 40)), (16384, (64, 2, 360))])
def test_category_counts_are_exact(cardinality, shape):
    from brainmagick_amd import hip_ops as H
    gen = torch.Generator().manual_seed(31 + cardinality)
    N, F, T = shape
    x = torch.randn(shape, generator=gen)
    cat = torch.randint(0, cardinality, (N, T), generator=gen)
    cat[0, 0] = 0
    cat[-1, -1] = cardinality - 1
    x[:, 1] = cat.float()
    for mask in (torch.rand(N, 1, T, generator=gen) > 0.4, torch.rand(N, F, T, generator=gen) > 0.4):
        sel = mask[:, 0] if mask.shape[1] == 1 else mask[:, 1]
        counts, flags = H.category_counts(x.to(DEV), mask.to(DEV), 1, cardinality)
        assert counts.dtype == torch.float32 and int(flags.item()) == 0
        assert torch.equal(counts.cpu(), torch.bincount(cat[sel], minlength=cardinality).float())


def test_category_counts_raise_the_flag_of_each_violation():
    from brainmagick_amd import hip_ops as H
    gen = torch.Generator().manual_seed(8)
    base = torch.randint(0, 5, (6, 1, 20), generator=gen).float()
    base[0, 0, 0] = 0
    mask = torch.ones(6, 1, 20, dtype=torch.bool)
    mask[2, 0, 7] = False                                   # the violations sit at a masked-OUT position

    def flags_of(value):
        x = base.clone()
        x[2, 0, 7] = value
        counts, flags = H.category_counts(x.to(DEV), mask.to(DEV), 0, 5)
        keep = base.clone().long()[mask]
        assert torch.equal(counts.cpu(), torch.bincount(keep, minlength=5).float())
        return int(flags.item())
    assert flags_of(1.0) == 0
    assert flags_of(1.5) == H.CATEGORY_NOT_INTEGER
    assert flags_of(5.0) == H.CATEGORY_MAX
    assert flags_of(-1.0) == H.CATEGORY_MIN
    assert flags_of(float("nan")) == H.CATEGORY_NOT_INTEGER
    assert flags_of(float("inf")) == H.CATEGORY_NOT_INTEGER | H.CATEGORY_MAX
    _, flags = H.category_counts((base + 1).to(DEV), mask.to(DEV), 0, 6)      # no zero anywhere: min != 0
    assert int(flags.item()) == H.CATEGORY_MIN
    with pytest.raises(ValueError, match="16384"):
        H.category_counts(base.to(DEV), mask.to(DEV), 0, 16385)


# ---- bm_center_scale_inverse ----------------------------------------------------------------------------------------
@pytest.mark.parametrize("T", [37, 40])
def test_center_scale_inverse_is_the_reference_expression(T):
    """(x * scale) + center with two roundings, grouped by recording and ungrouped, dword and vector path."""
    from brainmagick_amd import hip_ops as H
    gen = torch.Generator().manual_seed(T)
    x = torch.randn(7, 5, T, generator=gen) * 3
    center = torch.randn(3, 5, generator=gen)
    scale = torch.rand(3, 5, generator=gen) * 7 + 0.1
    group = torch.randint(0, 3, (7,), generator=gen)
    want = (x * scale[group][:, :, None]) + center[group][:, :, None]
    got = H.center_scale_inverse(x.to(DEV), center.to(DEV), scale.to(DEV), group=group.to(DEV))
    assert torch.equal(got.cpu().view(torch.int32), want.view(torch.int32))
    want = (x * scale[1][None, :, None]) + center[1][None, :, None]
    got = H.center_scale_inverse(x.to(DEV), center[1:2].to(DEV), scale[1:2].to(DEV))
    assert torch.equal(got.cpu().view(torch.int32), want.view(torch.int32))
    fused = torch.addcmul(center[1][None, :, None].double(), x.double(), scale[1][None, :, None].double()).float()
    assert not torch.equal(fused, want)                     # an FMA would be caught
