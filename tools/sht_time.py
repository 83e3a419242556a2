#!/usr/bin/env python
"""Time of the spherical-harmonic transforms (csrc/sht.hip, two launches per direction) against the reference's route restated on the GPU, and
of the O96 forward with the spectral Ornstein residual against the SkipConnection forward.  One process, fp32.

(a) transforms: O96 at truncation 95, O96 at truncation 191 (the residual's own: nlat - 1) and O8 (truncation 7), 1 field and 80 fields,
    forward and inverse.  ``kernel_us`` is device time from hipGraph replays (tools/gemm_sweep.timeit) of ``ops.sht_forward`` /
    ``ops.sht_inverse`` on the field-contiguous [F, grid] layout; ``kernel_columns_us`` (80 fields) the same call reading / writing 80 of 101
    columns of the model's [1, grid, 101] layout in place.  ``torch_us`` is the reference's route (layers/spectral_helpers.py:227-264, 317-340,
    448-477, 530-553) with torch ops: one torch.fft.rfft / irfft per ring into a zero-filled tensor, then two einsums over the dense fp32
    [m, l, k] table - timed by device events around back-to-back EAGER calls (its 192 launches per transform are what a user of the
    reference pays; ``torch_graph_us`` is the same route's device time from hipGraph replays where the capture succeeds, else null).  The
    two routes alternate and each is repeated; the spread is that of the repeats.  For the model layout the reference first copies the input
    to "(b t e v) p" order: ``torch_transpose_us``.
    Bytes: ``min_bytes`` is what the two launches must move at least - the fields, the ring spectra written and read once, the coefficients,
    and the Legendre table's lower triangle (l >= m) once per field tile; ``gbytes_per_s`` = min_bytes / kernel_us.
(b) model: the O96 -> res 5, 512-channel, 16-layer GraphTransformer forward (fp32, batch 1, 101 input columns of which 80 prognostic) with the
    SkipConnection and with SpectralOrnsteinConnection(lmax 8, octahedral, truncate, anti-aliasing, two regressors), hipGraph replays.

Writes one JSON (default profiles/r19_sht_time.json), rewritten after every row.
usage: python tools/sht_time.py [--out PATH] [--kernel-only] [--repeats R]"""
import argparse
import json
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from gemm_sweep import timeit  # noqa: E402

from anemoi_core_amd import ops  # noqa: E402
from anemoi_core_amd.layers.spectral_helpers import InverseSphericalHarmonicTransform, SphericalHarmonicTransform  # noqa: E402
from anemoi_core_amd.layers.spectral_transforms import octahedral_lons_per_lat  # noqa: E402

DEV = "cuda"
V, SELECTED, T = 101, 80, 2
SIZES = (("o96_t95", 192, 95), ("o96_t191", 192, 191), ("o8_t7", 16, 7))


def eager_time(fn, reps=10):
    for _ in range(2):
        fn()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    e0.record()
    for _ in range(reps):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) * 1e3 / reps


def torch_forward(x, lons, slon, weight, M):
    """The reference's forward route: per-ring rfft into a zero-filled [.., K, max n / 2 + 1] tensor, 2 pi, two einsums."""
    out = torch.zeros(*x.shape[:-1], len(lons), max(lons) // 2 + 1, device=x.device, dtype=torch.complex64)
    for i, (s, n) in enumerate(zip(slon, lons)):
        out[..., i, :n // 2 + 1] = torch.fft.rfft(x[..., s:s + n], norm="forward")
    xr = torch.view_as_real(2.0 * torch.pi * out)
    rl = torch.einsum("...km,mlk->...lm", xr[..., :M, 0], weight)
    im = torch.einsum("...km,mlk->...lm", xr[..., :M, 1], weight)
    return torch.view_as_complex(torch.stack((rl, im), -1))


def torch_inverse(c, lons, slon, pct):
    """The reference's inverse route: two einsums, then one irfft per ring into a zero-filled [.., grid] tensor."""
    cr = torch.view_as_real(c)
    rl = torch.einsum("...lm,mlk->...km", cr[..., 0], pct)
    im = torch.einsum("...lm,mlk->...km", cr[..., 1], pct)
    y = torch.view_as_complex(torch.stack((rl, im), -1))
    out = torch.zeros(*c.shape[:-2], sum(lons), device=c.device, dtype=torch.float32)
    for i, (s, n) in enumerate(zip(slon, lons)):
        out[..., s:s + n] = torch.fft.irfft(y[..., i, :], n, norm="forward")
    return out


def graph_time_or_none(fn):
    try:
        return timeit(fn, reps=2, replays=3)
    except Exception as e:  # noqa: BLE001  (rocFFT plans or the indexed writes may not capture: the eager figure stands alone then)
        print("torch route not captured:", type(e).__name__, str(e).splitlines()[0] if str(e) else "")
        torch.cuda.synchronize()
        return None


def min_bytes(direction, F, lons, trunc, field_tile):
    K, M, grid = len(lons), trunc + 1, sum(lons)
    table = 4 * K * M * (M + 1) // 2 * -(-F // field_tile)
    return 4 * F * grid + 2 * 8 * F * K * M + 8 * F * M * M + table


def transform_rows(repeats, rows, save, kernel_only):
    med = lambda v: sorted(v)[len(v) // 2]  # noqa: E731
    for name, nlat, trunc in SIZES:
        lons = octahedral_lons_per_lat(nlat)
        f, b = SphericalHarmonicTransform(lons, trunc).to(DEV), InverseSphericalHarmonicTransform(lons, trunc).to(DEV)
        w32, p32 = f.weight.float(), b.pct.float()
        L = trunc + 1
        for F in (1, SELECTED):
            g = torch.Generator(device=DEV).manual_seed(0)
            x = torch.randn(F, sum(lons), device=DEV, generator=g)
            c = torch.view_as_complex(torch.randn(F, L, L, 2, device=DEV, generator=g) * torch.tril(torch.ones(L, L, device=DEV))[..., None])
            wide = torch.randn(1, sum(lons), V, device=DEV, generator=g)
            cols = torch.arange(SELECTED, dtype=torch.int32, device=DEV)
            routes = {"forward": (lambda: f(x), lambda: torch_forward(x, lons, f.slon, w32, L)),
                      "inverse": (lambda: b(c), lambda: torch_inverse(c, lons, b.slon, p32))}
            for direction, (kern, ref) in routes.items():
                # results first: the two routes compute the same thing
                a, r = kern(), ref()
                a, r = (torch.view_as_real(a), torch.view_as_real(r)) if direction == "forward" else (a, r)
                diff = float((a - r).abs().max() / r.abs().max())
                kt, tt = [], []
                with torch.inference_mode():
                    for _ in range(repeats):
                        kt.append(timeit(kern, reps=10, replays=5))
                        if not kernel_only:
                            tt.append(eager_time(ref))
                    plan = ops.sht_plan(direction, F, lons, trunc)
                    row = dict(size=name, nlat=nlat, grid_points=sum(lons), truncation=trunc, fields=F, direction=direction, dtype="float32",
                               field_tile=plan["field_tile"], ring_lds_bytes=plan["lds_bytes"], max_rel_diff_to_torch_route=diff,
                               kernel_us=[round(t, 2) for t in kt], kernel_median_us=round(med(kt), 2))
                    nb = min_bytes(direction, F, lons, trunc, plan["field_tile"])
                    row.update(min_bytes=nb, gbytes_per_s=round(nb / med(kt) * 1e-3, 1))
                    if F == SELECTED:
                        if direction == "forward":
                            kc = [timeit(lambda: f(wide, cols=cols, columns=True), reps=10, replays=5) for _ in range(repeats)]
                            row["torch_transpose_us"] = round(med([timeit(lambda: wide.permute(0, 2, 1).contiguous(), reps=10, replays=5)
                                                                   for _ in range(repeats)]), 2)
                        else:
                            c4 = c.view(1, F, L, L)
                            kc = [timeit(lambda: b(c4, columns=True), reps=10, replays=5) for _ in range(repeats)]
                        row.update(kernel_columns_us=[round(t, 2) for t in kc], kernel_columns_median_us=round(med(kc), 2))
                    if not kernel_only:
                        tg = graph_time_or_none(ref)
                        row.update(torch_us=[round(t, 1) for t in tt], torch_median_us=round(med(tt), 1), torch_spread_us=round(max(tt) - min(tt), 1),
                                   torch_graph_us=None if tg is None else round(tg, 1), torch_over_kernel=round(med(tt) / med(kt), 1),
                                   torch_graph_over_kernel=None if tg is None else round(tg / med(kt), 1))
                print(json.dumps(row), flush=True)
                rows.append(row)
                save()


def model_rows(repeats, channels=512, layers=16, heads=16):
    from anemoi_core_amd.graphs.synthetic import build_synthetic_graph
    from anemoi_core_amd.models import AnemoiModelEncProcDec
    from anemoi_core_amd.models.configs import make_data_indices, model_config

    g = build_synthetic_graph("o96", 5)
    x = {"data": torch.randn(1, T, 1, g.num_data, V, device=DEV)}
    ornstein = {"_target_": "anemoi.models.layers.residual.SpectralOrnsteinConnection", "lmax": 8, "grid": "octahedral", "theta_init": 0.2,
                "theta_buff": 0.05, "regressors": [f"v{SELECTED}", f"v{SELECTED + 1}"], "truncate": True, "anti_aliasing": True}
    models = {}
    for name, residual in (("skip", None), ("ornstein", ornstein)):
        torch.manual_seed(0)
        models[name] = AnemoiModelEncProcDec(model_config=model_config("gt", channels, layers, heads, 8, residual=residual),
                                             data_indices=make_data_indices(V, SELECTED), statistics={"data": None}, n_step_input=T, n_step_output=1,
                                             graph_data=g).eval().to(DEV)
    skip_t, orn_t = [], []
    with torch.inference_mode():
        for _ in range(repeats):
            skip_t.append(timeit(lambda: models["skip"](x), reps=3, replays=5))
            orn_t.append(timeit(lambda: models["ornstein"](x), reps=3, replays=5))
        res = models["ornstein"].residual["data"]
        alone = [timeit(lambda: res.compact(x["data"][:, -1]), reps=10, replays=5) for _ in range(repeats)]
    med = lambda v: sorted(v)[len(v) // 2]  # noqa: E731
    row = dict(graph="o96 -> res 5", channels=channels, layers=layers, dtype="float32", batch=1, input_columns=V, prognostic_columns=SELECTED,
               residual=ornstein, skip_us=[round(t, 1) for t in skip_t], ornstein_us=[round(t, 1) for t in orn_t],
               skip_median_us=round(med(skip_t), 1), ornstein_median_us=round(med(orn_t), 1), skip_spread_us=round(max(skip_t) - min(skip_t), 1),
               added_us=round(med(orn_t) - med(skip_t), 1), residual_alone_us=[round(t, 1) for t in alone])
    print(json.dumps(row), flush=True)
    return row


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles", "r19_sht_time.json"))
    ap.add_argument("--kernel-only", action="store_true")
    ap.add_argument("--repeats", type=int, default=3)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("tools/sht_time.py measures on the GPU; none is visible")
    result = dict(device=torch.cuda.get_device_name(0), torch=torch.__version__, transforms=[])
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)

    def save():
        with open(args.out, "w") as fh:
            json.dump(result, fh, indent=1)

    transform_rows(args.repeats, result["transforms"], save, args.kernel_only)
    if not args.kernel_only:
        result["model"] = model_rows(args.repeats)
    save()
    print("wrote", args.out)


if __name__ == "__main__":
    main()
