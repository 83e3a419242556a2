"""Shared pieces of the ensemble-model tests: this package's AnemoiEnsModelEncProcDec built from a case of tests/golden/ens.pt (the
configuration, parameter draw and inputs of tests/golden/make_golden_ens.py) and the substitution of recorded noise."""
import os

import torch

from tests.transformer_helpers import GOLDEN, fill

N_CHANNELS, N_LAYERS, N_HEADS, TRAINABLE = 64, 2, 2, 8


def load_fixture() -> dict:
    return torch.load(os.path.join(GOLDEN, "ens.pt"), weights_only=False)


def config_of(case: dict, channels: int = N_CHANNELS, layers: int = N_LAYERS, heads: int = N_HEADS) -> dict:
    from anemoi_core_amd.models.configs import ens_model_config

    cfg = ens_model_config(case["kind"], channels, layers, heads, TRAINABLE, noise_channels_dim=4, noise_mlp_hidden_dim=32,
                           injector=case.get("injector", "NoiseConditioning"), condition_on_residual=case.get("condition_on_residual", False),
                           window_size=case.get("window_size", 512))
    if case["kind"] == "transformer":
        cfg["model"]["processor"]["attention_implementation"] = "scaled_dot_product_attention"
    return cfg


def ens_model(fx: dict, name: str):
    """(model, x, parameter checksum) of fixture case ``name``: parameters and inputs drawn as the generator drew them."""
    from anemoi_core_amd.graphs.synthetic import build_synthetic_graph
    from anemoi_core_amd.models import AnemoiEnsModelEncProcDec
    from anemoi_core_amd.models.configs import make_data_indices

    entry = fx[name]
    case = entry["case"]
    g = build_synthetic_graph("o8", 3, processor_edges=case["kind"] != "transformer")
    model = AnemoiEnsModelEncProcDec(model_config=config_of(case), data_indices=make_data_indices(fx["n_vars"], fx["n_vars"]),
                                     statistics={"data": None}, n_step_input=fx["n_step_input"], n_step_output=case.get("n_step_output", 1),
                                     graph_data=g).eval()
    psum = fill(model, entry["param_seed"])
    x = torch.randn(case.get("batch", 1), fx["n_step_input"], case["members"], g.num_data, fx["n_vars"],
                    generator=torch.Generator().manual_seed(entry["input_seed"]))
    return model, x, psum


def noise_conditioning(model):
    """The module whose ``draw`` produces the model's noise (the NoiseInjector wraps one)."""
    inj = model.noise_injector
    return getattr(inj, "_noise_conditioning", inj)


def fix_noise(model, noise: torch.Tensor) -> None:
    """Every forward of ``model`` draws ``noise`` ([batch, ensemble, grid, channels]) instead of fresh random numbers."""
    def draw(shape, dtype, device):
        assert tuple(shape) == tuple(noise.shape), (shape, noise.shape)
        return noise.to(device=device, dtype=dtype)

    noise_conditioning(model).draw = draw
