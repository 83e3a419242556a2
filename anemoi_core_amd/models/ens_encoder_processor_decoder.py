"""AnemoiEnsModelEncProcDec - mirror of the reference's ensemble model (models/src/anemoi/models/models/ens_encoder_processor_decoder.py
:34-322): the encoder / processor / decoder of ``AnemoiModelEncProcDec`` with the members of an ensemble folded into the batch dimension,
a forecast-step column (and optionally the residual's prognostic columns) appended to the encoder's input, and a ``noise_injector``
(layers/ensemble.py) between encoder and processor whose noise conditions the processor's ConditionalLayerNorms (``cond=``) or is
projected into the latent.

``forward(x: {name: [batch, time, ensemble, grid, vars]}, *, fcstep, model_comm_group=None, grid_shard_sizes=None)`` returns
``{name: [batch, n_step_output, ensemble, grid, vars]}``.  The model edges run the generic torch path of the base class (the fused
single-member assembly kernels stay where they are); every row-wise and GEMM launch in between is this library's.
"""
from __future__ import annotations

from typing import Optional

import torch
from torch import Tensor

from .. import ops
from ..distributed.primitives import scoped_forward, shard_tensor
from ..distributed.shapes import BipartiteGraphShardInfo, GraphShardInfo, comm_size, get_shard_sizes
from ..utils.config import DotDict, instantiate
from .encoder_processor_decoder import AnemoiModelEncProcDec, _retarget


class AnemoiEnsModelEncProcDec(AnemoiModelEncProcDec):
    """Message passing graph neural network with ensemble functionality."""

    def __init__(self, *, model_config, data_indices: dict, statistics: Optional[dict] = None, graph_data, n_step_input: int,
                 n_step_output: int) -> None:
        model_config = model_config if isinstance(model_config, DotDict) else DotDict(model_config)
        self.condition_on_residual = bool(model_config.model.condition_on_residual)
        super().__init__(model_config=model_config, data_indices=data_indices, statistics=statistics, graph_data=graph_data,
                         n_step_input=n_step_input, n_step_output=n_step_output)

    def _calculate_shapes_and_indices(self, data_indices: dict) -> None:
        super()._calculate_shapes_and_indices(data_indices)
        self.num_input_channels_prognostic = {ds: len(idx.model.input.prognostic) for ds, idx in data_indices.items()}
        for ds in data_indices:
            self.input_dim[ds] += 1  # for forecast step (fcstep)
            if self.condition_on_residual:
                self.input_dim[ds] += self.num_input_channels_prognostic[ds]
            self.target_dim[ds] = self.input_dim[ds]  # the decoder's destination rows are the encoder's input rows

    def _build_networks(self, mc, edges) -> None:
        super()._build_networks(mc, edges)
        self.noise_injector = instantiate(_retarget(mc.noise_injector), _recursive_=False, num_channels=self.num_channels)

    def _assemble_input(self, x: Tensor, fcstep: int, batch_ens_size: int, shard_sizes, group, ds: str):
        """ens_encoder_processor_decoder.py:75-118: [x rows | node attributes | fcstep | residual's columns]."""
        node_attr = self.node_attributes(ds, batch_size=batch_ens_size)
        if shard_sizes is not None:
            node_attr = shard_tensor(node_attr, 0, shard_sizes, group)
        B, T, E, N, V = x.shape
        x = x.to(node_attr.dtype)
        x_skip = x[:, self._skip_step, ...]  # SkipConnection: [batch, ensemble, grid, vars]; repeated over the output steps where it is added
        if self._truncated[ds]:  # TruncatedConnection: the prognostic columns only, coarse-grained and reconstructed (two launches)
            x_skip = self._truncated_skip(ds, x_skip, False, None, shard_sizes)
        flat = x.permute(0, 2, 3, 1, 4).reshape(B * E * N, T * V)  # "(batch ensemble grid) (time vars)"
        cols = [flat, node_attr, torch.full((B * E * N, 1), float(fcstep), dtype=flat.dtype, device=flat.device)]
        if self.condition_on_residual:
            cols.append(x_skip.reshape(B * E * N, -1))  # (the compact columns of a truncated residual)
        return torch.cat(cols, dim=-1), x_skip

    @scoped_forward
    def forward(self, x: dict, *, fcstep: int, model_comm_group=None, grid_shard_sizes: Optional[dict] = None, **kwargs) -> dict:
        names = list(x.keys())
        batch_size, ensemble_size = x[names[0]].shape[0], x[names[0]].shape[2]
        assert all(x[ds].shape[0] == batch_size and x[ds].shape[2] == ensemble_size for ds in names), "batch / ensemble sizes differ between datasets"
        batch_ens_size = batch_size * ensemble_size  # batch and ensemble dimensions are merged
        in_out_sharded = {ds: grid_shard_sizes is not None and grid_shard_sizes.get(ds) is not None for ds in names}
        assert not (any(in_out_sharded.values()) and model_comm_group is None), "If input is sharded, model_comm_group must be provided."
        if model_comm_group is not None and comm_size(model_comm_group) > 1:
            assert batch_size == 1, "Only batch size of 1 is supported when model is sharded across GPUs"
            assert ensemble_size == 1, "Ensemble size per device must be 1 when model is sharded across GPUs"
        fcstep = min(1, fcstep)
        hid = self._graph_name_hidden
        x_hidden_latent = self.node_attributes(hid, batch_size=batch_ens_size)
        shard_sizes_hidden = get_shard_sizes(x_hidden_latent, 0, model_comm_group)
        x_hidden_latent = shard_tensor(x_hidden_latent, 0, shard_sizes_hidden, model_comm_group)
        latents, skips, data_latents, data_shards = {}, {}, {}, {}
        for ds in names:
            data_shards[ds] = grid_shard_sizes[ds] if in_out_sharded[ds] else None
            x_data_latent, skips[ds] = self._assemble_input(x[ds], fcstep, batch_ens_size, data_shards[ds], model_comm_group, ds)
            ea, ei, es = self.encoder_graph_provider[ds].get_edges(batch_size=batch_ens_size, model_comm_group=model_comm_group)
            info = BipartiteGraphShardInfo(src_nodes=data_shards[ds], dst_nodes=shard_sizes_hidden, edges=es)
            data_latents[ds], latents[ds] = self.encoder[ds]((x_data_latent, x_hidden_latent.to(x_data_latent.dtype)), batch_size=batch_ens_size,
                                                             shard_info=info, edge_attr=ea, edge_index=ei, model_comm_group=model_comm_group,
                                                             keep_x_dst_sharded=True)
        x_latent = latents[names[0]] if len(names) == 1 else sum(latents.values())
        x_latent_proc, latent_noise = self.noise_injector(x=x_latent, batch_size=batch_size, ensemble_size=ensemble_size,
                                                          grid_size=self.node_attributes.num_nodes[hid], grid_shard_sizes=shard_sizes_hidden,
                                                          model_comm_group=model_comm_group)
        ea, ei, es = self.processor_graph_provider.get_edges(batch_size=batch_ens_size, model_comm_group=model_comm_group)
        x_latent_proc = self.processor(x=x_latent_proc, batch_size=batch_ens_size, shard_info=GraphShardInfo(nodes=shard_sizes_hidden, edges=es),
                                       edge_attr=ea, edge_index=ei, model_comm_group=model_comm_group,
                                       **({"cond": latent_noise} if latent_noise is not None else {}))
        if self.latent_skip:
            if x_latent_proc.is_cuda and x_latent_proc.shape == x_latent.shape and x_latent_proc.dtype == x_latent.dtype and not (
                    torch.is_grad_enabled() and (x_latent_proc.requires_grad or x_latent.requires_grad)):
                from ..layers.block import _identity_index  # inference: the add as one launch of this library

                x_latent_proc = ops.gather_add_rows(x_latent_proc, x_latent, _identity_index(x_latent))
            else:
                x_latent_proc = x_latent_proc + x_latent
        out = {}
        for ds in names:
            ea, ei, es = self.decoder_graph_provider[ds].get_edges(batch_size=batch_ens_size, model_comm_group=model_comm_group)
            info = BipartiteGraphShardInfo(src_nodes=shard_sizes_hidden, dst_nodes=data_shards[ds], edges=es)
            x_out = self.decoder[ds]((x_latent_proc, data_latents[ds]), batch_size=batch_ens_size, shard_info=info, edge_attr=ea, edge_index=ei,
                                     model_comm_group=model_comm_group, keep_x_dst_sharded=in_out_sharded[ds])
            # "(bs e n) (time vars) -> bs time e n vars", the residual on the prognostic columns, the boundings: the base class's generic path
            out[ds] = AnemoiModelEncProcDec._assemble_output(self, x_out, skips[ds], batch_size, ensemble_size, x[ds].dtype, ds,
                                                             compact=self._truncated[ds])
        return out

    def predict_step(self, *args, **kwargs):
        raise NotImplementedError("AnemoiEnsModelEncProcDec.predict_step: the ensemble rollout (fcstep per step, member handling) belongs to the "
                                  "ensemble forecaster; call forward(x, fcstep=...) with normalised inputs")
