"""Golden vectors of scaler fitting, from the REAL reference code (read-only /root/reference).

Run in the build container only:   python tests/golden/make_scaler_fit_golden.py [output directory]
Writes ``scaler_fit.npz`` (default: next to this file): the reference's ``BatchScaler.fit`` (bm/norm.py:152-237, loaded
unchanged; only its ``LogProgress`` name is replaced by a pass-through) on seeded lists of small batch objects.

  inputs   ``in/<loader>/<batch>/{meg,features,mask}`` and ``in/recording_index``: 3 recordings x 4 batches of 4
           segments, 6 sensors, T = 24; 4 normalizable feature channels ("emb") + 1 categorical channel ("cat",
           cardinality 5, category 3 absent) + 1 no-op channel ("aux"); masks [B, 1, T], about 60 % true.  The first
           recording has an all-constant sensor (scale -> 1), the second only values rounded to halves (ties).
           ``n_samples_per_recording = 10``: twelve segments per recording are taken, the fourth batch stays unread.
  cases    ``default`` (per_channel False), ``per_channel``, ``budget`` (n_samples_features = 20).  Per case:
           ``<case>/meg_center/<recording>``, ``<case>/meg_scale/<recording>``, ``<case>/emb_center``, ``<case>/emb_scale``
           (the reference's fp32 StandardScaler values), ``<case>/emb_center_f64``, ``<case>/emb_scale_f64`` (the same
           statistic of the same selected values in fp64 by numpy: the reference's own fp32 error is on record),
           ``<case>/cat_count``, ``<case>/cat_weights``, ``<case>/roundtrip/{meg,features}`` =
           inverse_transform(transform(batch)) of the batch ``roundtrip_in/*`` (segments of all three recordings).
  meta     JSON: shapes, and per case the batches the reference used -- ``meg`` {recording: [[loader, batch], ...]},
           ``features`` [[loader, batch], ...] in the order the reference concatenated them (read off the tensors its
           scalers received, not recomputed).
"""
import dataclasses
import json
import sys
from pathlib import Path

import numpy as np
import torch

HERE = Path(__file__).resolve().parent
sys.path.insert(0, str(HERE))

from _ref_import import load_reference_norm  # noqa: E402

DIMS = dict(recordings=3, batches=4, B=4, C=6, T=24, n_samples_per_recording=10, seed=5150)
RECORDING_INDEX = [2, 0, 1]                       # of loader 0, 1, 2
FEATURES = [("emb", 4, "normalizable", 0), ("cat", 1, "categorical", 5), ("aux", 1, "noop", 0)]
CASES = {"default": dict(per_channel=False), "per_channel": dict(per_channel=True),
         "budget": dict(per_channel=False, n_samples_features=20)}


@dataclasses.dataclass
class Batch:
    meg: torch.Tensor
    features: torch.Tensor
    features_mask: torch.Tensor
    recording_index: torch.Tensor

    def replace(self, **kw):
        return dataclasses.replace(self, **kw)


@dataclasses.dataclass
class Feature:
    normalizable: bool
    categorical: bool
    cardinality: int


class Builder:
    """The surface of bm.features.FeaturesBuilder that bm/norm.py touches."""

    def __init__(self, spec=FEATURES):
        self.features, self.slices, start = {}, {}, 0
        for name, dim, kind, cardinality in spec:
            self.features[name] = Feature(kind == "normalizable", kind == "categorical", cardinality)
            self.slices[name] = slice(start, start + dim)
            start += dim
        self.dimension = start

    def items(self):
        return self.features.items()

    def get_slice(self, name):
        return self.slices[name]


def make_loaders():
    d = DIMS
    gen = torch.Generator().manual_seed(d["seed"])
    B, C, T = d["B"], d["C"], d["T"]
    loaders = []
    for li in range(d["recordings"]):
        batches = []
        for bi in range(d["batches"]):
            gain = torch.logspace(-1, 1, C)[None, :, None]
            meg = torch.randn(B, C, T, generator=gen) * gain + torch.arange(C)[None, :, None] * 0.25
            if li == 0:
                meg[:, 4] = 0.0                           # a padded sensor: all quantiles equal, scale -> 1
            if li == 1:
                meg = torch.round(meg * 2) / 2            # heavy ties
            emb = torch.randn(B, 4, T, generator=gen) * torch.tensor([0.5, 1.0, 2.0, 4.0])[None, :, None] \
                + torch.tensor([-1.0, 0.0, 3.0, 10.0])[None, :, None]
            cat = torch.tensor([0., 1., 2., 4.])[torch.randint(0, 4, (B, 1, T), generator=gen)]
            aux = torch.rand(B, 1, T, generator=gen)
            mask = torch.rand(B, 1, T, generator=gen) > 0.4
            batches.append(Batch(meg, torch.cat([emb, cat, aux], 1), mask,
                                 torch.full((B,), RECORDING_INDEX[li], dtype=torch.long)))
        loaders.append(batches)
    return loaders


class Recorded:
    """A loader that remembers which of its batches were asked for."""

    def __init__(self, batches):
        self.batches, self.seen = batches, []

    def __iter__(self):
        for bi, batch in enumerate(self.batches):
            self.seen.append(bi)
            yield batch


def build() -> dict:
    torch.set_num_threads(1)          # the reference's CPU reductions in one fixed order: regeneration is bit-exact
    norm = load_reference_norm()
    norm.LogProgress = lambda logger, iterable, **kw: iterable
    d = DIMS
    T = d["T"]
    loaders = make_loaders()
    out = {"in/recording_index": np.asarray(RECORDING_INDEX, dtype=np.int64)}
    for li, batches in enumerate(loaders):
        for bi, b in enumerate(batches):
            out[f"in/{li}/{bi}/meg"] = b.meg.numpy().copy()
            out[f"in/{li}/{bi}/features"] = b.features.numpy().copy()
            out[f"in/{li}/{bi}/mask"] = b.features_mask.numpy().copy()
    # a batch with segments of every recording, for the round trip
    rt = Batch(torch.cat([loaders[li][3].meg[:2] for li in range(3)]),
               torch.cat([loaders[li][3].features[:2] for li in range(3)]),
               torch.cat([loaders[li][3].features_mask[:2] for li in range(3)]),
               torch.cat([loaders[li][3].recording_index[:2] for li in range(3)]))
    out["roundtrip_in/meg"] = rt.meg.numpy().copy()
    out["roundtrip_in/features"] = rt.features.numpy().copy()
    out["roundtrip_in/mask"] = rt.features_mask.numpy().copy()
    out["roundtrip_in/recording_index"] = rt.recording_index.numpy().copy()

    meta = dict(dims=d, features=[list(f) for f in FEATURES], cases={}, torch=torch.__version__)
    real_fit = norm.StandardScaler.fit
    for case, kw in CASES.items():
        builder = Builder()
        recorded = [Recorded(b) for b in loaders]
        seen = {}

        def spy(self, X, mask, _seen=seen):
            _seen["X"], _seen["mask"] = X.clone(), mask.clone()
            return real_fit(self, X, mask)
        norm.StandardScaler.fit = spy
        try:
            scaler = norm.BatchScaler(builder, n_samples_per_recording=d["n_samples_per_recording"], **kw)
            scaler.fit(recorded)
        finally:
            norm.StandardScaler.fit = real_fit
        for rec, sc in scaler.meg_scalers.items():
            out[f"{case}/meg_center/{rec}"] = sc.center_.numpy().copy()
            out[f"{case}/meg_scale/{rec}"] = sc.scale_.numpy().copy()
        emb = scaler.feature_scalers["emb"]
        out[f"{case}/emb_center"] = np.asarray(emb.center_.numpy(), dtype=np.float32).copy()
        out[f"{case}/emb_scale"] = np.asarray(emb.scale_.numpy(), dtype=np.float32).copy()
        X, mask = seen["X"].double().numpy(), seen["mask"].numpy()[:, 0]          # [samples, 4], [samples]
        picked = X[mask]
        if kw["per_channel"]:
            out[f"{case}/emb_center_f64"] = picked.mean(0)
            out[f"{case}/emb_scale_f64"] = picked.std(0, ddof=1)
        else:
            out[f"{case}/emb_center_f64"] = np.asarray(picked.mean())
            out[f"{case}/emb_scale_f64"] = np.asarray(picked.std(ddof=1))
        out[f"{case}/cat_count"] = scaler.feature_scalers["cat"].categories_count_.numpy().copy()
        out[f"{case}/cat_weights"] = scaler.get_categorical_feature_weights("cat").numpy().copy()
        back = scaler.inverse_transform(scaler.transform(rt))
        out[f"{case}/roundtrip/meg"] = back.meg.numpy().copy()
        out[f"{case}/roundtrip/features"] = back.features.numpy().copy()
        # which batches: the loaders' own record, and the feature rows the reference handed to its scalers
        used_meg = {str(RECORDING_INDEX[li]): [[li, bi] for bi in r.seen] for li, r in enumerate(recorded)}
        rows = seen["X"].view(-1, T, 4).permute(0, 2, 1)                          # [segments, 4, T]
        used_features = []
        for k in range(0, len(rows), d["B"]):
            match = [[li, bi] for li, batches in enumerate(loaders) for bi, b in enumerate(batches)
                     if torch.equal(b.features[:, :4], rows[k:k + d["B"]])]
            assert len(match) == 1, (case, k, match)
            used_features.append(match[0])
        meta["cases"][case] = dict(kwargs=kw, meg=used_meg, features=used_features)
    out["meta"] = json.dumps(meta)
    return out


def main(argv):
    dest = Path(argv[0]) if argv else HERE
    dest.mkdir(parents=True, exist_ok=True)
    out = build()
    np.savez_compressed(dest / "scaler_fit.npz", **out)
    print(f"scaler_fit: {len(out)} arrays -> {dest / 'scaler_fit.npz'}")


if __name__ == "__main__":
    main(sys.argv[1:])
