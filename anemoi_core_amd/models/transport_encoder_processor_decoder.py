"""AnemoiTransportModelEncProcDec - mirror of the reference's transport (diffusion) model
(models/src/anemoi/models/models/transport_encoder_processor_decoder.py:47-645) for the ``edm_diffusion`` objective, state prediction: the
encoder / processor / decoder of ``AnemoiModelEncProcDec`` whose ConditionalLayerNorms are conditioned on the noise level, with the
noised target appended to the encoder's input.  Same constructor keywords, attributes (``noise_embedder``, ``noise_cond_mlp``, ``edm``,
``noise_conditioning``, ``transport_source``, ``inference_defaults``) and state_dict keys.

``forward(x, conditioned_target, condition, ...)``: x {name: [batch, time, ensemble, grid, vars]}, the noised target
{name: [batch, n_step_output, ensemble, grid, output vars]} and sigma {name: [batch, 1, ensemble, 1, 1]} -> the denoised state.

Around the network run exactly three launches of this library per dataset (ops.noise_cond, ops.transport_assemble_input,
ops.edm_output); no torch operation touches the state.  Ensemble members are folded into the batch, as in the ensemble model (the
reference builds the hidden attributes for ``batch_size`` rows, :291, and fails on more than one member).

Training: under autograd the three launches run as ``autograd.NoiseCondFunction`` / ``TransportAssembleInputFunction`` /
``EdmOutputFunction`` (backward kernels: csrc/transport_bwd.hip), the network takes the trainable routes of its blocks, and
``prepare_edm_training`` draws sigma from ``training_condition``, noises the target and returns the EDM loss weights; the loss itself stays
with the caller.  Gradients reach every parameter; the noise level, the noised target and x carry none (refused by name).

Not implemented, each refused with a message that names it: the tendency model, the stochastic-interpolant objective, a sharded model or
grid, GNN / Transformer processors or mappers inside the transport model, differentiating through a sampler.  ``predict_step`` calls the
pre- and post-processor modules (no fused normaliser / imputer chain)."""
from __future__ import annotations

from typing import Optional

import torch
from torch import Tensor, nn

from .. import ops
from ..distributed.primitives import scoped_forward
from ..distributed.shapes import BipartiteGraphShardInfo, GraphShardInfo, comm_size, get_shard_sizes
from ..transport import (SIGMA_TRAINING_DISTRIBUTIONS, EdmSettings, NoiseConditioningSettings, TransportSourceBuilder, TransportSourceSpec,
                         edm_loss_weight, get_transport_model_objective, sampling_source_specs)
from ..utils.config import DotDict, instantiate
from .encoder_processor_decoder import _PAD64, AnemoiModelEncProcDec, _retarget


class AnemoiTransportModelEncProcDec(AnemoiModelEncProcDec):
    """Encoder-processor-decoder model conditioned on the diffusion noise level."""

    def __init__(self, *, model_config, data_indices: dict, statistics: Optional[dict] = None, n_step_input: int, n_step_output: int,
                 graph_data) -> None:
        model_config = model_config if isinstance(model_config, DotDict) else DotDict(model_config)
        tp = model_config.model.model.transport
        self.noise_conditioning = NoiseConditioningSettings.from_config(tp)
        self.edm = EdmSettings.from_config(tp)
        self.transport_source = TransportSourceBuilder.from_config(tp)
        self.training_condition = dict(tp.get("training_condition", {}) or {})
        self.noise_channels, self.noise_cond_dim = self.noise_conditioning.channels, self.noise_conditioning.cond_dim
        self.inference_defaults = tp.get("inference_defaults", {}) or {}
        self.transport_model_objective = get_transport_model_objective(tp.objective)
        if self.noise_channels % 2 or not (2 <= self.noise_channels <= ops.NOISE_CHANNELS_MAX and 1 <= self.noise_cond_dim <= ops.NOISE_COND_MAX):
            raise NotImplementedError(f"transport model: noise_channels={self.noise_channels} (even, <= {ops.NOISE_CHANNELS_MAX}) and "
                                      f"noise_cond_dim={self.noise_cond_dim} (<= {ops.NOISE_COND_MAX}) are what the noise-conditioning kernel takes")
        super().__init__(model_config=model_config, data_indices=data_indices, statistics=statistics, graph_data=graph_data,
                         n_step_input=n_step_input, n_step_output=n_step_output)
        self.noise_embedder = instantiate(_retarget(tp.noise_embedder))
        if not hasattr(self.noise_embedder, "embedding_operands"):
            raise NotImplementedError(f"transport model: noise embedder {type(self.noise_embedder).__name__} is not implemented; supported: "
                                      "RandomFourierEmbeddings, SinusoidalEmbeddings (layers/diffusion.py)")
        self.noise_cond_mlp = self._create_noise_conditioning_mlp()

    def _calculate_shapes_and_indices(self, data_indices: dict) -> None:
        super()._calculate_shapes_and_indices(data_indices)
        for ds in data_indices:
            self.input_dim[ds] += self.output_dim[ds]  # input history plus the corrupted target
            self.target_dim[ds] = self.input_dim[ds]

    def _build_networks(self, mc, edges) -> None:
        from ..layers.mapper import GraphTransformerBackwardMapper, GraphTransformerForwardMapper
        from ..layers.processor import GraphTransformerProcessor

        super()._build_networks(mc, edges)
        for ds in self.dataset_names:
            if not (isinstance(self.encoder[ds], GraphTransformerForwardMapper) and isinstance(self.decoder[ds], GraphTransformerBackwardMapper)):
                raise NotImplementedError("transport model: GNN and Transformer mappers inside the transport model are not implemented; use the "
                                          "GraphTransformer mappers")
        if not isinstance(self.processor, GraphTransformerProcessor):
            raise NotImplementedError(f"transport model: a {type(self.processor).__name__} inside the transport model is not implemented; use the "
                                      "GraphTransformerProcessor")

    def _create_noise_conditioning_mlp(self) -> nn.Sequential:
        mlp = nn.Sequential()
        mlp.add_module("linear1_no_gradscaling", nn.Linear(self.noise_channels, self.noise_channels))
        mlp.add_module("activation", nn.SiLU())
        mlp.add_module("linear2_no_gradscaling", nn.Linear(self.noise_channels, self.noise_cond_dim))
        return mlp

    def cast_network(self, dtype) -> "AnemoiTransportModelEncProcDec":
        """Cast the network to a 16-bit ``dtype`` and leave the noise embedder in fp32: its ``frequencies`` multiply noise levels into
        arguments of hundreds of radians, where a 16-bit frequency is a different phase (``model.to(dtype)`` would round them)."""
        for name, child in self.named_children():
            if name != "noise_embedder":
                child.to(dtype)
        return self

    # -- conditioning ---------------------------------------------------------------------------------------------------
    @staticmethod
    def _assert_condition_shapes(condition: dict) -> tuple:
        ref = next(iter(condition.values()))
        assert ref.ndim == 5, "Expected condition to have shape (batch, 1, ensemble, 1, 1)."
        batch_size, _, ensemble_size = ref.shape[:3]
        for ds, c in condition.items():
            assert c.ndim == 5 and c.shape[1] == c.shape[3] == c.shape[4] == 1, f"Expected condition to have shape (batch, 1, ensemble, 1, 1) for '{ds}'."
            assert c.shape[0] == batch_size and c.shape[2] == ensemble_size, "Batch or ensemble dimension mismatch across datasets for conditioned inputs."
        return batch_size, ensemble_size

    def _noise_rows(self, values: Tensor, log_quarter: bool, rows: tuple, dtype) -> tuple:
        """The conditioning of ``values`` [groups] repeated over ``rows[k]`` nodes per group: one launch (embedder + MLP + both repeats)."""
        freq, pi = self.noise_embedder.embedding_operands()
        l1, l2 = self.noise_cond_mlp.linear1_no_gradscaling, self.noise_cond_mlp.linear2_no_gradscaling
        return ops.noise_cond(values, freq.float(), l1.weight, l1.bias, l2.weight, l2.bias, pi=None if pi is None else pi.float(),
                              log_quarter=log_quarter, rows=rows, out_dtype=dtype)

    def _embed_noise_conditioning(self, sigma: Tensor) -> Tensor:
        """noise_cond_mlp(noise_embedder(sigma)) for sigma [..., 1] -> [..., noise_cond_dim]."""
        out, = self._noise_rows(sigma.reshape(-1), False, (1,), self.noise_cond_mlp.linear2_no_gradscaling.weight.dtype)
        return out.view(*sigma.shape[:-1], self.noise_cond_dim)

    def _input_width(self, ds: str, cols: int, dtype) -> int:
        """The assembled rows carry the alignment zeros of the embedding GEMM's K dimension (the base model's rule)."""
        if dtype == torch.float32 or not self._prepad(ds):
            return cols
        return cols + ((-cols) % 64 if (-cols) % 64 <= 16 and _PAD64 else (-cols) % 8)

    # -- forward ----------------------------------------------------------------------------------------------------------
    @scoped_forward
    def forward(self, x: dict, conditioned_target: dict, condition: dict, model_comm_group=None, grid_shard_sizes: Optional[dict] = None,
                **kwargs) -> dict:
        return self.transport_model_objective.forward(self, x, conditioned_target, condition, model_comm_group=model_comm_group,
                                                      grid_shard_sizes=grid_shard_sizes, **kwargs)

    def _forward_transport_network(self, x: dict, conditioned_target: dict, condition: dict, model_comm_group=None,
                                   grid_shard_sizes: Optional[dict] = None, edm=None, out_dtype=None, **kwargs) -> dict:
        """The network on [x | conditioned_target | node attributes] conditioned on ``condition``.  ``edm`` (an EdmSettings): ``condition``
        is sigma and the EDM preconditioning is applied at the edges - log(sigma) / 4 conditions the network, the target is scaled by
        c_in, the result is c_skip target + c_out output.  ``out_dtype``: float32 (default: x's dtype) or float64."""
        names = list(x.keys())
        batch_size, ensemble_size = x[names[0]].shape[0], x[names[0]].shape[2]
        assert all(x[ds].shape[0] == batch_size and x[ds].shape[2] == ensemble_size for ds in names), "batch / ensemble sizes differ between datasets"
        if (model_comm_group is not None and comm_size(model_comm_group) > 1) or (
                grid_shard_sizes is not None and any(grid_shard_sizes.get(ds) is not None for ds in names)):
            raise NotImplementedError("transport model: a sharded model or grid (model_comm_group of more than one rank, grid_shard_sizes) is "
                                      "not implemented")
        self._assert_condition_shapes(condition)
        bse = batch_size * ensemble_size  # batch and ensemble dimensions are merged
        hid = self._graph_name_hidden
        n_nodes = self.node_attributes.num_nodes
        x_hidden_latent = self._hidden_attributes(bse)
        dtype = x_hidden_latent.dtype  # the model dtype
        # one noise level per sample and member, shared by the datasets: read from the first
        sigma = condition[names[0]].reshape(-1)
        rows, c_data, c_hidden = {}, {}, None
        for ds in names:
            xd, yd = x[ds], conditioned_target[ds]
            c_data[ds], c_h = self._noise_rows(sigma, edm is not None, (n_nodes[ds], n_nodes[hid] if c_hidden is None else 0), dtype)
            c_hidden = c_h if c_hidden is None else c_hidden
            attrs = self.node_attributes(ds, batch_size=1)
            cols = xd.shape[1] * xd.shape[4] + yd.shape[1] * yd.shape[4] + attrs.shape[1]
            assert cols == self.input_dim[ds], f"'{ds}': {cols} input columns, the model was built for {self.input_dim[ds]}"
            rows[ds] = ops.transport_assemble_input(xd, yd, attrs, self._input_width(ds, cols, dtype), sigma=sigma if edm is not None else None,
                                                    sigma_data=edm.sigma_data if edm is not None else 1.0, out_dtype=dtype)
        x_out = self._run_network(rows, c_data, c_hidden, bse, model_comm_group)
        out = {}
        for ds in names:
            yd = conditioned_target[ds]
            out[ds] = ops.edm_output(x_out[ds], yd if edm is not None else None, sigma if edm is not None else None, tuple(yd.shape),
                                     sigma_data=edm.sigma_data if edm is not None else 1.0, out_dtype=out_dtype or x[ds].dtype)
        return out

    def _run_network(self, rows: dict, c_data: dict, c_hidden: Tensor, bse: int, model_comm_group=None) -> dict:
        """Encoder, processor (+ latent skip) and decoder on assembled input rows {name: [bse grid, width]} with the conditioning rows of the
        data nodes {name: [bse grid, cond]} and of the hidden nodes -> the decoder's output rows {name: [bse grid, time vars]}."""
        names = list(rows)
        x_hidden_latent = self._hidden_attributes(bse)
        shard_sizes_hidden = get_shard_sizes(x_hidden_latent, 0, model_comm_group)
        latents, data_latents = {}, {}
        for ds in names:
            ea, ei, es = self.encoder_graph_provider[ds].get_edges(batch_size=bse, model_comm_group=model_comm_group)
            info = BipartiteGraphShardInfo(src_nodes=None, dst_nodes=shard_sizes_hidden, edges=es)
            data_latents[ds], latents[ds] = self.encoder[ds]((rows[ds], x_hidden_latent), batch_size=bse, shard_info=info, edge_attr=ea,
                                                             edge_index=ei, model_comm_group=model_comm_group, keep_x_dst_sharded=True,
                                                             cond=(c_data[ds], c_hidden))
        x_latent = latents[names[0]] if len(names) == 1 else sum(latents.values())
        ea, ei, es = self.processor_graph_provider.get_edges(batch_size=bse, model_comm_group=model_comm_group)
        x_latent_proc = self.processor(x=x_latent, batch_size=bse, shard_info=GraphShardInfo(nodes=shard_sizes_hidden, edges=es), edge_attr=ea,
                                       edge_index=ei, model_comm_group=model_comm_group, cond=c_hidden)
        if self.latent_skip:
            if torch.is_grad_enabled() and (x_latent_proc.requires_grad or x_latent.requires_grad):
                x_latent_proc = x_latent_proc + x_latent  # training: the differentiable add (the ensemble model's route)
            else:
                from ..layers.block import _identity_index  # inference: the add as one launch of this library

                x_latent_proc = ops.gather_add_rows(x_latent_proc, x_latent, _identity_index(x_latent))
        out = {}
        for ds in names:
            ea, ei, es = self.decoder_graph_provider[ds].get_edges(batch_size=bse, model_comm_group=model_comm_group)
            info = BipartiteGraphShardInfo(src_nodes=shard_sizes_hidden, dst_nodes=None, edges=es)
            out[ds] = self.decoder[ds]((x_latent_proc, data_latents[ds]), batch_size=bse, shard_info=info, edge_attr=ea, edge_index=ei,
                                       model_comm_group=model_comm_group, keep_x_dst_sharded=False, cond=(c_hidden, c_data[ds]))
        return out

    # -- training ---------------------------------------------------------------------------------------------------------
    def prepare_edm_training(self, target: dict, source: Optional[dict] = None, sigma: Optional[dict] = None) -> tuple:
        """What one EDM training step feeds the model and its loss - the reference's EDMDiffusionTransportObjective.prepare
        (training/train/methods/edm_diffusion.py:28-51): (y_noised, sigma, weights), each {name: tensor}, from the clean ``target``
        {name: [batch, n_step_output, ensemble, grid, output vars]}.  sigma [batch, 1, ensemble, 1, 1]: one draw per sample and member from the
        distribution ``training_condition`` names, shared by the datasets; source: ``transport_source`` (Gaussian by default);
        y_noised = target + source sigma; weights = edm_loss_weight(sigma, sigma_data).  ``source`` / ``sigma`` given: used as they are.
        Torch operations on the device of ``target``; the loss, mean(weights (model(x, y_noised, sigma) - target)^2), stays with the caller."""
        if sigma is None:
            config = dict(self.training_condition)
            try:
                name = config.pop("distribution")
            except KeyError as exc:
                raise ValueError("EDM training_condition must define 'distribution'.") from exc
            if name not in SIGMA_TRAINING_DISTRIBUTIONS:
                raise ValueError(f"Unknown EDM training condition distribution: {name}")
            sigma = SIGMA_TRAINING_DISTRIBUTIONS[name](**config).sample({ds: tuple(t.shape) for ds, t in target.items()},
                                                                      device=next(iter(target.values())).device)
        weights = {ds: edm_loss_weight(s, self.edm.sigma_data) for ds, s in sigma.items()}
        if source is None:
            specs = {ds: TransportSourceSpec(shape=tuple(t.shape), device=t.device, dtype=t.dtype) for ds, t in target.items()}
            source = self.transport_source.build(specs, default_kind="gaussian", error_context="training")
        y_noised = {ds: target[ds] + source[ds] * sigma[ds] for ds in target}
        return y_noised, sigma, weights

    # -- sampling ---------------------------------------------------------------------------------------------------------
    def build_sampling_source(self, x: dict, model_comm_group=None, grid_shard_sizes: Optional[dict] = None, default_kind: str = "gaussian") -> dict:
        """The field sampling starts from: {name: [batch, n_step_output, ensemble, grid, output vars]} in x's dtype."""
        specs = sampling_source_specs(x, n_step_output=self.n_step_output, num_output_channels=self.num_output_channels,
                                      grid_shard_sizes=grid_shard_sizes)
        return self.transport_source.build(specs, default_kind=default_kind, error_context="state prediction")

    def sample(self, x: dict, model_comm_group=None, grid_shard_sizes: Optional[dict] = None, schedule_params: Optional[dict] = None,
               sampler_params: Optional[dict] = None, **kwargs) -> dict:
        """Run the sampler selected by the transport objective (``inference_defaults`` overridden by the two dicts)."""
        return self.transport_model_objective.sample(self, x, model_comm_group=model_comm_group, grid_shard_sizes=grid_shard_sizes,
                                                     schedule_params=schedule_params, sampler_params=sampler_params, **kwargs)

    def predict_step(self, batch: dict, pre_processors, post_processors, n_step_input: int, model_comm_group=None, gather_out: bool = True,
                     schedule_params: Optional[dict] = None, sampler_params: Optional[dict] = None, **kwargs) -> dict:
        """Pre-process, sample, post-process: ``batch[ds]`` is [batch, time, grid, vars] of raw data."""
        if model_comm_group is not None and comm_size(model_comm_group) > 1:
            raise NotImplementedError("transport model: predict_step with a sharded model (model_comm_group of more than one rank) is not implemented")
        with torch.no_grad():
            assert isinstance(batch, dict), "Input batch must be a dictionary!"
            x = {}
            for ds, t in batch.items():
                assert t.dim() == 4, f'The input tensor "{ds}" has an incorrect shape: expected a 4-dimensional tensor, got {t.shape}!'
                x[ds] = pre_processors[ds](t[:, 0:n_step_input, None, ...], in_place=False)  # dummy ensemble dimension as 3rd index
            out = self.sample(x, model_comm_group, grid_shard_sizes=None, schedule_params=schedule_params, sampler_params=sampler_params)
            return {ds: post_processors[ds](out[ds].to(batch[ds].dtype), in_place=False) for ds in out}

    def fill_metadata(self, md_dict) -> None:
        for ds in self.input_dim:
            md_dict["metadata_inference"][ds]["shapes"] = {"variables": self.input_dim[ds], "input_timesteps": self.n_step_input, "ensemble": 1,
                                                           "grid": None}  # (the grid size is dynamic)


class AnemoiTransportTendModelEncProcDec:
    """The tendency-predicting transport model of the reference (transport_encoder_processor_decoder.py:647-1047): not implemented."""

    def __init__(self, *args, **kwargs) -> None:
        raise NotImplementedError("AnemoiTransportTendModelEncProcDec (transport on tendencies, with its per-step tendency processors) is not "
                                  "implemented; AnemoiTransportModelEncProcDec predicts states")
