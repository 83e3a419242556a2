"""Config / index builders for the benchmark and the tests: the nested ``model_config`` the reference's
AnemoiModelEncProcDec is instantiated from (training/src/anemoi/training/config/model/graphtransformer.yaml) and a
minimal ``data_indices`` object (models/tests/models/test_base_graph_model.py:33-56)."""
from types import SimpleNamespace


class IndexGroup(SimpleNamespace):
    def __len__(self):
        return len(self.full)


def make_data_indices(n_vars_in, n_prog):
    names = {f"v{i}": i for i in range(n_vars_in)}
    prog = list(range(n_prog))
    ns = SimpleNamespace(
        model=SimpleNamespace(
            input=IndexGroup(prognostic=prog, full=list(range(n_vars_in)), name_to_index=names),
            output=IndexGroup(prognostic=prog, full=prog, diagnostic=[], name_to_index={f"v{i}": i for i in prog}),
            _forcing=[],
        ),
        data=SimpleNamespace(input=SimpleNamespace(name_to_index=names)),
        name_to_index=names,
    )
    return {"data": ns}


def model_config(kind, num_channels, num_layers, num_heads, trainable, prefix="anemoi.models.layers", window_size=512, residual=None):
    """Same nested config the reference model is built from (tests/golden/make_golden.py); by default it even carries
    the REFERENCE's ``_target_`` strings, which the model retargets to the MI355X classes.  ``kind``: "gt", "gnn" or "transformer"
    (GraphTransformer mappers around a TransformerProcessor with ``window_size``, the reference's transformer.yaml; its graph needs no
    hidden -> hidden edges).  ``residual``: the ``model.residual`` entry (default: the SkipConnection of the last step), e.g.
    ``truncated_residual_config()``."""
    common = dict(cpu_offload=False, gradient_checkpointing=False, layer_kernels=None, trainable_size=trainable,
                  sub_graph_edge_attributes=["edge_length", "edge_dirs"])
    if kind == "transformer":
        common.update(num_heads=num_heads, mlp_hidden_ratio=4, qk_norm=False, mlp_implementation="mlp")
        mapper = dict(common, shard_strategy="edges", graph_attention_backend="triton", edge_pre_mlp=False)
        enc = dict(mapper, _target_=f"{prefix}.mapper.GraphTransformerForwardMapper", num_chunks=2)
        dec = dict(mapper, _target_=f"{prefix}.mapper.GraphTransformerBackwardMapper", num_chunks=2, initialise_data_extractor_zero=False)
        proc = dict(common, _target_=f"{prefix}.processor.TransformerProcessor", num_chunks=1, num_layers=num_layers, window_size=window_size,
                    dropout_p=0.0, attention_implementation="flash_attention", softcap=0.0, use_alibi_slopes=False, use_rotary_embeddings=False)
        proc.pop("sub_graph_edge_attributes")
        proc.pop("trainable_size")
    elif kind == "gt":
        common.update(num_heads=num_heads, mlp_hidden_ratio=4, qk_norm=False, shard_strategy="edges",
                      graph_attention_backend="pyg", edge_pre_mlp=False)
        enc = dict(common, _target_=f"{prefix}.mapper.GraphTransformerForwardMapper", num_chunks=2)
        proc = dict(common, _target_=f"{prefix}.processor.GraphTransformerProcessor", num_chunks=1, num_layers=num_layers)
        dec = dict(common, _target_=f"{prefix}.mapper.GraphTransformerBackwardMapper", num_chunks=2, initialise_data_extractor_zero=False)
    else:
        common.update(mlp_extra_layers=0)
        enc = dict(common, _target_=f"{prefix}.mapper.GNNForwardMapper", num_chunks=1)
        proc = dict(common, _target_=f"{prefix}.processor.GNNProcessor", num_chunks=1, num_layers=num_layers)
        dec = dict(common, _target_=f"{prefix}.mapper.GNNBackwardMapper", num_chunks=1)
    return {
        "model": {
            "num_channels": num_channels,
            "trainable_parameters": {"data": trainable, "hidden": trainable, "data2hidden": trainable, "hidden2data": trainable, "hidden2hidden": trainable},
            "model": {"hidden_nodes_name": "hidden", "latent_skip": True},
            "encoder": enc, "processor": proc, "decoder": dec,
            "residual": dict(residual) if residual is not None else {"_target_": "anemoi.models.layers.residual.SkipConnection", "step": -1},
            "bounding": [],
        }
    }


def truncated_residual_config(prefix="anemoi.models.layers", *, data="data", truncation="truncation", edge_weight_attribute=None,
                              src_node_weight_attribute=None, row_normalize=False, **extra):
    """The ``model.residual`` entry of a TruncatedConnection over pre-resolved edge sets (training config model/residual: truncated)."""
    return dict({"_target_": f"{prefix}.residual.TruncatedConnection", "truncation_down_edges_name": (data, "to", truncation),
                 "truncation_up_edges_name": (truncation, "to", data), "edge_weight_attribute": edge_weight_attribute,
                 "src_node_weight_attribute": src_node_weight_attribute, "autocast": False, "row_normalize": row_normalize}, **extra)


def ens_model_config(kind, num_channels, num_layers, num_heads, trainable, *, noise_channels_dim=4, noise_mlp_hidden_dim=32, noise_std=1,
                     injector="NoiseConditioning", condition_on_residual=False, prefix="anemoi.models.layers", window_size=512, residual=None):
    """The nested config of the reference's AnemoiEnsModelEncProcDec (training/src/anemoi/training/config/model/graphtransformer_ens.yaml,
    transformer_ens.yaml): ``model_config(kind, ...)`` ("gt" or "transformer") plus ``condition_on_residual`` and the ``noise_injector``.
    ``injector``: "NoiseConditioning" (the noise conditions the processor, whose ``layer_kernels.LayerNorm`` becomes a ConditionalLayerNorm of
    ``condition_shape = noise_channels_dim``), "NoiseInjector" (projected into the latent; plain LayerNorms) or "NoOpNoiseInjector"."""
    cfg = model_config(kind, num_channels, num_layers, num_heads, trainable, prefix=prefix, window_size=window_size, residual=residual)
    m = cfg["model"]
    m["condition_on_residual"] = condition_on_residual
    inj = {"_target_": f"{prefix}.ensemble.{injector}"}
    if injector != "NoOpNoiseInjector":
        inj.update(noise_std=noise_std, noise_channels_dim=noise_channels_dim, noise_mlp_hidden_dim=noise_mlp_hidden_dim, noise_matrix=None,
                   layer_kernels=None)
    if injector == "NoiseConditioning":
        inj.update(noise_edges_name=None, edge_weight_attribute=None, row_normalize_noise_matrix=False, autocast=False)
        m["processor"]["layer_kernels"] = {"LayerNorm": {"_target_": f"{prefix}.normalization.ConditionalLayerNorm", "_partial_": True,
                                                         "condition_shape": noise_channels_dim, "zero_init": True, "autocast": False}}
    m["noise_injector"] = inj
    return cfg


def transport_model_config(kind, num_channels, num_layers, num_heads, trainable, *, noise_embedder="SinusoidalEmbeddings", noise_channels=32,
                           noise_cond_dim=16, objective="edm_diffusion", sigma_data=1.0, sigma_max=100.0, sigma_min=0.02, rho=7.0, source=None,
                           inference_defaults=None, training_condition=None, prefix="anemoi.models.layers", **embedder_kw):
    """The nested config of the reference's AnemoiTransportModelEncProcDec (training/src/anemoi/training/config/model/
    graphtransformer_transport_edm.yaml): ``model_config(kind, ...)`` whose encoder, processor and decoder take a ConditionalLayerNorm of
    ``condition_shape = noise_cond_dim`` as ``layer_kernels.LayerNorm``, plus the ``model.model.transport`` section.  ``noise_embedder``:
    "SinusoidalEmbeddings" (``max_period``) or "RandomFourierEmbeddings" (``scale``) of layers/diffusion.py; ``inference_defaults``:
    {"sampling_schedule": {"schedule_type": ..., ...}, "sampler": {"sampler": ..., ...}}; ``training_condition``: {"distribution": one of
    transport.SIGMA_TRAINING_DISTRIBUTIONS, its keywords ...}, what ``prepare_edm_training`` draws sigma from (absent when None)."""
    cfg = model_config(kind, num_channels, num_layers, num_heads, trainable, prefix=prefix)
    m = cfg["model"]
    for part in ("encoder", "processor", "decoder"):
        m[part]["layer_kernels"] = {"LayerNorm": {"_target_": f"{prefix}.normalization.ConditionalLayerNorm", "_partial_": True,
                                                  "condition_shape": noise_cond_dim, "zero_init": True, "autocast": False}}
    if inference_defaults is None:
        inference_defaults = {"sampling_schedule": {"schedule_type": "karras", "sigma_max": sigma_max, "sigma_min": sigma_min, "rho": rho,
                                                    "num_steps": 20},
                              "sampler": {"sampler": "heun", "S_churn": 0.0, "S_min": 0.0, "S_max": float("inf"), "S_noise": 1.0}}
    m["model"]["transport"] = {"objective": objective, "noise_channels": noise_channels, "noise_cond_dim": noise_cond_dim,
                               "noise_embedder": dict({"_target_": f"{prefix}.diffusion.{noise_embedder}", "num_channels": noise_channels}, **embedder_kw),
                               "sigma_data": sigma_data, "sigma_max": sigma_max, "sigma_min": sigma_min, "rho": rho, "source": dict(source or {}),
                               "inference_defaults": inference_defaults}
    if training_condition is not None:
        m["model"]["transport"]["training_condition"] = dict(training_condition)
    return cfg
