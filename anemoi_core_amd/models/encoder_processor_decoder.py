"""AnemoiModelEncProcDec — mirror of the reference glue (models/src/anemoi/models/models/encoder_processor_decoder.py
:33-340 and models/base.py:38-395) for the graph (GraphTransformer / GNN) model family: same constructor arguments,
``forward(x: {name: [B,T,E,N,V]}, model_comm_group=None, grid_shard_sizes=None)`` and state_dict keys
(``encoder.<ds>.*``, ``processor.*``, ``decoder.<ds>.*``, ``node_attributes.*``, ``*_graph_provider.*``).

``model_config`` is the reference's nested config (attribute dict).  ``_target_`` strings may name either this
package's classes or the reference's ``anemoi.models.layers.*`` classes (rewritten to the MI355X implementations), so an
existing config selects the HIP path without edits.  Residual: ``model.residual`` is instantiated per dataset as the reference does
(models/base.py:244-258) - SkipConnection (step) or TruncatedConnection (layers/residual.py; any other target raises); boundings: all
eight classes of layers/bounding.py, run as one in-place column program.
"""
from __future__ import annotations

import os
from typing import NamedTuple, Optional

import torch
from torch import Tensor, nn

from .. import ops
from ..distributed.primitives import scoped_forward, shard_tensor
from ..distributed.shapes import BipartiteGraphShardInfo, GraphShardInfo, comm_size, get_shard_sizes
from ..layers.graph import NamedNodesAttributes
from ..layers.graph_provider import create_graph_provider
from ..layers.mapper import GraphTransformerBaseMapper
from ..utils.tensors import version

_FUSED_INPUT = os.environ.get("ANEMOI_FUSED_INPUT", "1") == "1"  # developer switch: 0 = permute-copy + cat in torch
_PAD64 = os.environ.get("ANEMOI_PAD64", "1") == "1"  # developer switch: 0 = pad the input width to a multiple of 8 only
# the decoder block's k|v projection of the hidden rows at the end of the last processor block's chain launch (ANEMOI_TAIL_KV=0: LayerNorm launch + GEMM)
_TAIL_KV = os.environ.get("ANEMOI_TAIL_KV", "1") != "0"
# The decoder's destination side (emb_nodes_dst -> layer_norm_attention_dest -> q|self over the data rows) reads nothing but the assembled input:
# its 48-row panels ride on the compute units the encoder's and the processor's block tails leave idle (layers/handoff.py SideJob,
# csrc/gt_chain2.hip SIDE) instead of standing as launches of their own behind the last processor layer.  ANEMOI_SIDE_JOB=0: off - the path is
# then exactly the one without it.  ANEMOI_SIDE_PANELS_PER_RIDER: panels per idle compute unit and round of a hosting launch.
_SIDE_JOB = os.environ.get("ANEMOI_SIDE_JOB", "1") != "0"
_SIDE_PANELS_PER_RIDER = int(os.environ.get("ANEMOI_SIDE_PANELS_PER_RIDER", "4"))
LAST_SIDE_JOB_PANELS = None  # developer aid / tests: (panels hosted, panels left over) of the last forward's side job; None: it had none
from ..utils.config import DotDict, instantiate

_REF_PREFIX = "anemoi.models.layers."
_OUR_PREFIX = "anemoi_core_amd.layers."


class _EdgeState(NamedTuple):
    """What one dataset's input assembly hands to its output assembly within a forward."""
    x_skip: Tensor
    skip_is_raw: bool
    norm_in: Optional[nn.Module]
    norm_out: Optional[nn.Module]
    imputer: Optional[nn.Module]
    nan_mask: Optional[Tensor]  # bool [N, V] when the imputation program ran inside the assembly kernel, else None
    remapper: Optional[nn.Module] = None  # the chain's Remapper: its inverse is part of the output column program
    remap_fused: bool = False  # the remap program ran inside the assembly kernel: the raw skip is not remapped either
    post_members: Optional[list] = None  # the members of the post chain when it holds more than [imputer, normaliser]


def _retarget(cfg) -> dict:
    cfg = dict(cfg)
    t = cfg.get("_target_", "")
    if isinstance(t, str) and t.startswith(_REF_PREFIX):
        cfg["_target_"] = _OUR_PREFIX + t[len(_REF_PREFIX):]
    return cfg


def _graph_views(graph_data):
    """Accept the synthetic generator's ``SyntheticGraph`` or a HeteroData-like object (``g[name].x``,
    ``g[(src,'to',dst)].edge_index / edge_length / edge_dirs``).  Returns (node coordinates by name, edge stores by type, the graph the
    residual connection is built from): a HeteroData-like graph or a ``graphs/io.GraphData`` is handed to the residual as it is - it reads the
    truncation node set (``num_nodes``, node attributes) and the truncation edge stores with their weight attribute by name; a
    ``SyntheticGraph`` has no such sets (None)."""
    if hasattr(graph_data, "enc_edge_index"):  # SyntheticGraph
        g = graph_data
        nodes = {"data": torch.as_tensor(g.data_latlon), "hidden": torch.as_tensor(g.hidden_latlon)}
        mk = lambda ei, ea: {"edge_index": torch.as_tensor(ei), "edge_length": torch.as_tensor(ea[:, :1]), "edge_dirs": torch.as_tensor(ea[:, 1:])}  # noqa: E731
        edges = {("data", "to", "hidden"): mk(g.enc_edge_index, g.enc_edge_attr),
                 ("hidden", "to", "hidden"): None if g.proc_edge_index is None else mk(g.proc_edge_index, g.proc_edge_attr),
                 ("hidden", "to", "data"): mk(g.dec_edge_index, g.dec_edge_attr)}
        return nodes, edges, None

    class _Edges(dict):
        def __missing__(self, key):
            # an edge type the graph does not have (e.g. no hidden -> hidden edges for a TransformerProcessor): None, so that the
            # provider is a NoOpGraphProvider, as in the reference
            types = getattr(graph_data, "edge_types", None)
            if types is not None and key not in types:
                return None
            return graph_data[key]

    nodes = {name: torch.as_tensor(graph_data[name].x) for name in graph_data.node_types}
    return nodes, _Edges(), graph_data


class AnemoiModelEncProcDec(nn.Module):
    def __init__(self, *, model_config, data_indices: dict, statistics: Optional[dict] = None, n_step_input: int,
                 n_step_output: int, graph_data) -> None:
        super().__init__()
        model_config = model_config if isinstance(model_config, DotDict) else DotDict(model_config)
        mc = model_config.model
        self.data_indices = data_indices
        self.statistics = statistics
        self.n_step_input = n_step_input
        self.n_step_output = n_step_output
        self.dataset_names = list(data_indices.keys())
        self._graph_name_hidden = mc.model.hidden_nodes_name
        self.num_channels = mc.num_channels
        self.latent_skip = mc.model.latent_skip
        if not isinstance(self._graph_name_hidden, str):
            raise NotImplementedError("hierarchical hidden node lists belong to another model family")
        nodes, edges, residual_graph = _graph_views(graph_data)
        tp = dict(mc.trainable_parameters)
        self.node_attributes = NamedNodesAttributes(
            {**{ds: tp.get("data", 0) for ds in self.dataset_names}, self._graph_name_hidden: tp.get("hidden", 0)},
            {**{ds: nodes[ds] for ds in self.dataset_names}, self._graph_name_hidden: nodes[self._graph_name_hidden]},
        )
        self._calculate_shapes_and_indices(data_indices)
        self._build_networks(mc, edges)
        self._build_residual(mc, residual_graph, nodes)
        self.boundings = self._build_boundings(mc.get("bounding", []) or [])
        self._pad_zeros = self._hidden_padded = None
        self._bound_tables: dict = {}

    # -- shapes (models/base.py:96-150) -------------------------------------------------------------------
    def _calculate_shapes_and_indices(self, data_indices: dict) -> None:
        self.num_input_channels, self.num_output_channels = {}, {}
        self._internal_input_idx, self._internal_output_idx = {}, {}
        self.input_dim, self.target_dim, self.output_dim = {}, {}, {}
        self.input_dim_latent = self.node_attributes.attr_ndims[self._graph_name_hidden]
        for ds, idx in data_indices.items():
            self._internal_input_idx[ds] = list(idx.model.input.prognostic)
            self._internal_output_idx[ds] = list(idx.model.output.prognostic)
            self.num_input_channels[ds] = len(idx.model.input)
            self.num_output_channels[ds] = len(idx.model.output)
            self.input_dim[ds] = self.n_step_input * self.num_input_channels[ds] + self.node_attributes.attr_ndims[ds]
            self.target_dim[ds] = self.input_dim[ds]
            self.output_dim[ds] = self.n_step_output * self.num_output_channels[ds]
            assert len(self._internal_input_idx[ds]) == len(self._internal_output_idx[ds])
            # device-resident index vectors (non-persistent: the state_dict stays identical to the reference's) so that
            # the residual scatter involves no host->device copy and the forward is hipGraph-capturable
            self.register_buffer(f"_in_idx_{ds}", torch.tensor(self._internal_input_idx[ds], dtype=torch.long), persistent=False)
            self.register_buffer(f"_out_idx_{ds}", torch.tensor(self._internal_output_idx[ds], dtype=torch.long), persistent=False)
            cmap = None
            if len(set(self._internal_output_idx[ds])) == len(self._internal_output_idx[ds]):  # one residual per output column
                cmap = torch.full((self.num_output_channels[ds],), -1, dtype=torch.int32)
                cmap[torch.tensor(self._internal_output_idx[ds], dtype=torch.long)] = torch.tensor(self._internal_input_idx[ds], dtype=torch.int32)
            self.register_buffer(f"_col_map_{ds}", cmap, persistent=False)

    def _build_networks(self, mc, edges) -> None:
        hid = self._graph_name_hidden
        n = self.node_attributes.num_nodes
        self.encoder_graph_provider, self.encoder = nn.ModuleDict(), nn.ModuleDict()
        for ds in self.dataset_names:
            self.encoder_graph_provider[ds] = create_graph_provider(
                graph=edges[(ds, "to", hid)], edge_attributes=mc.encoder.get("sub_graph_edge_attributes"),
                src_size=n[ds], dst_size=n[hid], trainable_size=mc.encoder.get("trainable_size", 0))
            self.encoder[ds] = instantiate(_retarget(mc.encoder), _recursive_=False, in_channels_src=self.input_dim[ds],
                                           in_channels_dst=self.input_dim_latent, hidden_dim=self.num_channels,
                                           edge_dim=self.encoder_graph_provider[ds].edge_dim)
        self.processor_graph_provider = create_graph_provider(
            graph=edges[(hid, "to", hid)], edge_attributes=mc.processor.get("sub_graph_edge_attributes"),
            src_size=n[hid], dst_size=n[hid], trainable_size=mc.processor.get("trainable_size", 0))
        self.processor = instantiate(_retarget(mc.processor), _recursive_=False, num_channels=self.num_channels,
                                     edge_dim=self.processor_graph_provider.edge_dim)
        self.decoder_graph_provider, self.decoder = nn.ModuleDict(), nn.ModuleDict()
        for ds in self.dataset_names:
            self.decoder_graph_provider[ds] = create_graph_provider(
                graph=edges[(hid, "to", ds)], edge_attributes=mc.decoder.get("sub_graph_edge_attributes"),
                src_size=n[hid], dst_size=n[ds], trainable_size=mc.decoder.get("trainable_size", 0))
            self.decoder[ds] = instantiate(_retarget(mc.decoder), _recursive_=False, in_channels_src=self.num_channels,
                                           in_channels_dst=self.target_dim[ds], hidden_dim=self.num_channels,
                                           out_channels_dst=self.output_dim[ds], edge_dim=self.decoder_graph_provider[ds].edge_dim)

    def _build_residual(self, mc, graph, nodes=None) -> None:
        """models/base.py:244-258: ``model.residual`` instantiated per dataset.  An absent or empty entry is the SkipConnection of the last
        step.  A TruncatedConnection gets the device-resident column vectors of its compact skip: the prognostic input columns it projects and
        the map from output column to compact column (non-persistent buffers: nothing is added to the state_dict); so does a
        SpectralOrnsteinConnection, whose skip is compact as well (``_truncated`` = the skip is the compact normalised one).  It reads the data
        nodes' coordinates only, so a graph without residual node sets hands it ``nodes`` (name -> coordinates)."""
        from ..layers.residual import SkipConnection, SpectralOrnsteinConnection, TruncatedConnection

        cfg = mc.get("residual", None) or {}
        chunks = (mc.get("sparse_projector", None) or {}).get("num_chunks", 1)
        self.residual = nn.ModuleDict()
        for ds in self.dataset_names:
            if not cfg or "_target_" not in cfg:
                self.residual[ds] = SkipConnection(step=int(cfg.get("step", -1)))
                continue
            target = _retarget(cfg)["_target_"]
            if target not in (_OUR_PREFIX + "residual.SkipConnection", _OUR_PREFIX + "residual.TruncatedConnection",
                              _OUR_PREFIX + "residual.SpectralOrnsteinConnection"):
                raise NotImplementedError(f"residual '{cfg['_target_']}' is not implemented; supported: SkipConnection, TruncatedConnection, "
                                          "SpectralOrnsteinConnection (layers/residual.py)")
            stats = self.statistics.get(ds) if isinstance(self.statistics, dict) else self.statistics
            ornstein = target.endswith("SpectralOrnsteinConnection")
            self.residual[ds] = instantiate(_retarget(cfg), _recursive_=False, graph=nodes if ornstein and graph is None else graph, data_node_name=ds if len(self.dataset_names) > 1 else "data",
                                            statistics=stats, data_indices=self.data_indices[ds], dataset_name=ds,
                                            sparse_projector_num_chunks=chunks)
            if isinstance(self.residual[ds], (TruncatedConnection, SpectralOrnsteinConnection)):
                out_idx, in_idx = self._internal_output_idx[ds], self._internal_input_idx[ds]
                cmap = torch.full((self.num_output_channels[ds],), -1, dtype=torch.int32)
                cmap[torch.tensor(out_idx, dtype=torch.long)] = torch.arange(len(out_idx), dtype=torch.int32)
                self.register_buffer(f"_col_map_c_{ds}", cmap if len(set(out_idx)) == len(out_idx) else None, persistent=False)
                self.register_buffer(f"_prog_cols_{ds}", torch.tensor(in_idx, dtype=torch.int32), persistent=False)
        first = self.residual[self.dataset_names[0]]
        self._skip_step = int(first.step) if isinstance(first, SkipConnection) else -1
        self._ornstein = {ds: isinstance(self.residual[ds], SpectralOrnsteinConnection) for ds in self.dataset_names}
        self._truncated = {ds: isinstance(self.residual[ds], TruncatedConnection) or self._ornstein[ds] for ds in self.dataset_names}
        self._skip_programs: dict = {}

    def _truncated_skip(self, ds: str, x_last: Tensor, raw: bool, norm, shard_sizes) -> Tensor:
        """The truncated residual of one forward: x_last [batch, ensemble, grid, vars] (the last input step, read in place) -> the
        NORMALISED compact skip [batch, ensemble, grid, prognostic columns].  ``raw``: x_last is the raw batch (``predict_step`` fused the
        input normaliser), whose column program then runs on every value the down projection gathers."""
        if self._ornstein[ds]:
            raise NotImplementedError("SpectralOrnsteinConnection is wired into AnemoiModelEncProcDec only (its forward computes the skip "
                                      "before the input assembly); the ensemble model does not support it yet")
        if shard_sizes is not None:
            raise NotImplementedError("TruncatedConnection with a sharded data grid (grid_shard_sizes) needs the reference's grid-to-channel "
                                      "transposes (layers/residual.py:287-293) and is not implemented; pass the whole grid")
        cols = getattr(self, f"_prog_cols_{ds}")
        mul = add = None
        if raw:
            # one entry per (dataset, device), replaced when the normaliser or its state changes.  The gather below runs on the first
            # forward with that normaliser: run one eager predict_step before capturing it, as for the bounding tables.
            slot, state = (ds, str(x_last.device)), (id(norm), norm._norm_mul._version, norm._norm_add._version)
            hit = self._skip_programs.get(slot)
            if hit is None or hit[0] != state:
                m, a = norm.column_program(x_last.shape[-1])
                hit = self._skip_programs[slot] = (state, (m[cols.long()].contiguous(), a[cols.long()].contiguous()))
            mul, add = hit[1]
        return self.residual[ds].project(x_last, cols=cols, mul=mul, add=add)

    def _build_boundings(self, cfgs) -> nn.ModuleDict:
        """models/base.py:94-97 / layers/bounding.py:312-400: one ModuleList per dataset, configuration order."""
        from ..layers.bounding import build_boundings_for

        out = nn.ModuleDict()
        for ds in self.dataset_names:
            stats = self.statistics.get(ds) if isinstance(self.statistics, dict) else self.statistics
            out[ds] = build_boundings_for(cfgs, self.data_indices[ds].model.output.name_to_index, stats,
                                          self.data_indices[ds].data.input.name_to_index)
        return out

    # -- glue (encoder_processor_decoder.py:98-163) ---------------------------------------------------------
    def _assemble_input(self, x: Tensor, batch_size: int, shard_sizes, group, ds: str, norm=None, imputer=None, remapper=None):
        """``norm``: the dataset's InputNormalizer when ``predict_step`` fuses it (x is then the RAW batch); ``imputer`` / ``remapper``: the
        imputer and the Remapper that precede it in the chain.  Returns (x_data_latent, x_skip, skip_is_raw, nan_mask, remap_fused):
        nan_mask bool [N, V], the NaN locations of the first step, when the imputation program ran inside the assembly kernel (the skip is
        then raw AND not imputed), else None; remap_fused: the remap program ran there as well (the raw skip is not remapped)."""
        node_attr = self.node_attributes(ds, batch_size=batch_size)
        if shard_sizes is not None:
            node_attr = shard_tensor(node_attr, 0, shard_sizes, group)
        B, T, E, N, V = x.shape
        fusable = (_FUSED_INPUT and B == 1 and E == 1 and x.is_cuda and x.stride(4) == 1
                   and not (torch.is_grad_enabled() and (x.requires_grad or node_attr.requires_grad)))
        if imputer is not None or remapper is not None:
            # the programs ride in the assembly kernels for one sample, one output step, the step skip and a whole grid; everything else
            # (a batch, several output steps, a truncated residual - whose down projection would need the programs on every gathered value -,
            # a sharded grid, training) runs the stand-alone kernels first, ONE pass per member (no host synchronisation: the domain
            # assertion belongs to the chain's first-batch check), and goes on as if the chain were the normaliser alone
            if not (fusable and self.n_step_output == 1 and not self._truncated[ds] and shard_sizes is None and not torch.is_grad_enabled()
                    and (node_attr.dtype == x.dtype or x.dtype == torch.float32)):
                fresh = imputer is not None
                if fresh:
                    x, imputer = imputer.transform(x, in_place=False), None
                if remapper is not None:
                    x, remapper = remapper.transform(x if x.stride(-1) == 1 else x.contiguous(), in_place=fresh, check_domain=False), None
            else:
                width = T * V + node_attr.shape[1]
                if node_attr.dtype != torch.float32 and self._prepad(ds):
                    width += (-width) % 64 if (-width) % 64 <= 16 and _PAD64 else (-width) % 8
                nan_mask = None if imputer is None else torch.empty((N, V), dtype=torch.bool, device=x.device)
                mul, add = norm.column_program(V)
                out = ops.assemble_input(x[0, :, 0], node_attr, width, mul, add, out_dtype=node_attr.dtype,
                                         impute=None if imputer is None else imputer.device_program(V, x.dtype, x.device), nan_mask=nan_mask,
                                         remap=None if remapper is None else remapper.device_program(V, False, x.device)[0])
                return out, x[:, self._skip_step, ...], True, nan_mask, remapper is not None
        if fusable and (node_attr.dtype == x.dtype or (norm is not None and x.dtype == torch.float32)):
            # inference, one member: permute + cat + alignment zeros (+ the input normaliser as a column program) in ONE kernel
            width = T * V + node_attr.shape[1]
            if node_attr.dtype != torch.float32 and self._prepad(ds):
                width += (-width) % 64 if (-width) % 64 <= 16 and _PAD64 else (-width) % 8
            if norm is None:
                return ops.assemble_input(x[0, :, 0], node_attr, width), x[:, self._skip_step, ...], False, None, False
            mul, add = norm.column_program(V)
            return ops.assemble_input(x[0, :, 0], node_attr, width, mul, add, out_dtype=node_attr.dtype), x[:, self._skip_step, ...], True, None, False
        if norm is not None:  # not fusable: the normaliser's own kernel, then the generic path
            x = norm.transform(x, in_place=False).to(node_attr.dtype)
        x_skip = x[:, self._skip_step, ...]  # SkipConnection (layers/residual.py:60-81): last input step
        flat = x.permute(0, 2, 3, 1, 4).reshape(B * E * N, T * V)  # "(batch ensemble grid) (time vars)"
        cols = [flat, node_attr.to(flat.dtype)]
        width = flat.shape[1] + node_attr.shape[1]
        pad = (-width) % 64 if (-width) % 64 <= 16 and _PAD64 else (-width) % 8  # a K multiple of 64 takes the DMA-ring GEMM kernels
        if pad and flat.dtype != torch.float32 and self._prepad(ds):
            # 16-bit GEMM operand rows must be 16-byte aligned: the zero columns the embeddings of encoder (source) and decoder
            # (destination) would each append with a pad kernel are written by this cat instead (PaddedLinear takes such rows)
            key = (flat.shape[0], pad, flat.dtype, str(flat.device))
            if self._pad_zeros is None or self._pad_zeros[0] != key:
                self._pad_zeros = (key, torch.zeros((flat.shape[0], pad), dtype=flat.dtype, device=flat.device))
            cols.append(self._pad_zeros[1])
        return torch.cat(cols, dim=-1), x_skip, False, None, False

    def _prepad(self, ds: str) -> bool:
        """The GraphTransformer mappers embed their inputs through PaddedLinear, which accepts rows that already carry the
        alignment zeros; the GNN mappers (MLP embeddings) take the exact width."""
        return isinstance(self.encoder[ds], GraphTransformerBaseMapper) and isinstance(self.decoder[ds], GraphTransformerBaseMapper)

    def _hidden_attributes(self, batch_size: int) -> Tensor:
        """Node attributes of the hidden mesh; outside training (a static tensor) with the zero columns of the 16-byte row
        alignment already appended, once."""
        x = self.node_attributes(self._graph_name_hidden, batch_size=batch_size)
        # a handful of attribute columns: pad K to 64 (a static [N_hidden, 64] tensor) so that the hidden-node embedding takes the
        # DMA-ring kernels and can emit the row statistics of the encoder's destination LayerNorm
        pad = (-x.shape[1]) % 64 if _PAD64 and x.shape[1] < 64 else (-x.shape[1]) % 8
        if not pad or x.dtype == torch.float32 or (torch.is_grad_enabled() and x.requires_grad) or not all(self._prepad(ds) for ds in self.dataset_names):
            return x
        key = (x.data_ptr(), version(x), tuple(x.shape), x.dtype)
        if self._hidden_padded is None or self._hidden_padded[0] != key:
            self._hidden_padded = (key, torch.nn.functional.pad(x, (0, pad)), x)
        return self._hidden_padded[1]

    def _assemble_output(self, x_out: Tensor, x_skip: Tensor, batch_size: int, ensemble_size: int, dtype, ds: str, norm=None,
                         skip_is_raw: bool = False, denorm=None, compact: bool = False, imputer=None, nan_mask: Optional[Tensor] = None,
                         remapper=None, remap_fused: bool = False, post_members: Optional[list] = None) -> Tensor:
        """``norm`` / ``skip_is_raw``: x_skip is the RAW input and is normalised inside the residual kernel; ``denorm``: the
        output InputNormalizer whose inverse transform is appended to the column program of the boundings; ``compact``: x_skip holds the
        prognostic columns only, in their order (the truncated residual); ``imputer`` / ``nan_mask`` (from ``_assemble_input``): the raw skip
        is imputed by the imputer's program as well, and its NaN restoration (op 10, reading nan_mask) closes the column program.
        ``remapper`` / ``remap_fused``: the raw skip goes through the remap program as well; ``post_members``: the members of a post chain
        with a Remapper or post-processors - the output program is then the boundings followed by every member's inverse ops, last member
        first (``ops.column_program_``)."""
        N = x_out.shape[0] // (batch_size * ensemble_size)
        in_idx, out_idx = getattr(self, f"_in_idx_{ds}"), getattr(self, f"_out_idx_{ds}")
        col_map = getattr(self, f"_col_map_c_{ds}" if compact else f"_col_map_{ds}")
        fusable = (col_map is not None and batch_size == 1 and ensemble_size == 1 and self.n_step_output == 1 and x_out.is_cuda
                   and not (torch.is_grad_enabled() and (x_out.requires_grad or x_skip.requires_grad)))
        fused_norm = fusable and skip_is_raw and x_skip.dtype == dtype and dtype in (x_out.dtype, torch.float32)
        program = None if nan_mask is None else imputer.device_program(x_skip.shape[-1], x_skip.dtype, x_skip.device)
        remap = remapper.device_program(x_skip.shape[-1], False, x_skip.device)[0] if remap_fused else None
        if skip_is_raw and not fused_norm:  # every path but the fused-normalisation kernel takes a NORMALISED (imputed, remapped) skip
            if program is not None:
                x_skip = ops.impute_columns(x_skip.unsqueeze(1), program).squeeze(1)
            if remap is not None:
                x_skip = ops.remap_columns((x_skip if x_skip.stride(-1) == 1 else x_skip.contiguous()).unsqueeze(1), remap,
                                           out=x_skip.unsqueeze(1) if program is not None else None).squeeze(1)
            x_skip, skip_is_raw = norm.transform(x_skip, in_place=program is not None or remap is not None), False
        if fused_norm:
            mul, add = norm.column_program(x_skip.shape[-1])
            x_out = ops.assemble_output(x_out, x_skip.reshape(N, -1), col_map, mul, add, impute=program, remap=remap).view(1, 1, 1, N, -1)
        elif fusable and x_out.dtype == dtype and x_skip.dtype == dtype:
            # one kernel for cast / residual on the prognostic columns (instead of clone + index_select + index_add_)
            x_out = ops.assemble_output(x_out, x_skip.reshape(N, -1), col_map).view(1, 1, 1, N, -1)
        else:
            x_out = x_out.reshape(batch_size, ensemble_size, N, self.n_step_output, -1).permute(0, 3, 1, 2, 4).to(dtype=dtype).clone()
            # SkipConnection._expand_time (layers/residual.py:53-57): the skip is repeated over the output steps
            skip = x_skip.unsqueeze(1).expand(-1, self.n_step_output, -1, -1, -1)
            x_out.index_add_(-1, out_idx, (skip if compact else skip.index_select(-1, in_idx)).to(dtype))
        if post_members is not None:
            return self._extended_output_program(x_out, ds, post_members, imputer, nan_mask)
        nan_ops = [] if nan_mask is None else imputer.inverse_program(x_out.shape[-1])
        if len(self.boundings[ds]) or denorm is not None or nan_ops:
            # all configured boundings (configuration order) and, fused, the output de-normalisation as ONE in-place column program
            from ..layers.bounding import apply_program_torch, masked_program_tables, program_tables

            if torch.is_grad_enabled() and x_out.requires_grad:
                x_out = apply_program_torch(x_out, [op for b in self.boundings[ds] for op in b.program()])
                if denorm is not None:
                    x_out = denorm.inverse_transform(x_out, in_place=False)
                if nan_ops:
                    x_out = imputer.inverse_transform(x_out, in_place=False)
            else:
                # the column program and its device tables are built ONCE per (dataset, device, normaliser state): program() of
                # the normalised boundings reads a registered buffer (.tolist() = a device->host sync, illegal under hipGraph capture)
                key = (ds, str(x_out.device), None if denorm is None else (id(denorm), denorm._norm_mul._version, denorm._norm_add._version))
                if nan_ops:
                    key += (id(imputer),)
                if key not in self._bound_tables:
                    prog = [op for b in self.boundings[ds] for op in b.program()]
                    if denorm is not None:
                        prog += denorm.inverse_program(x_out.shape[-1])
                    # (NaN restoration last: it follows the de-normalisation)
                    self._bound_tables[key] = masked_program_tables(prog + nan_ops, x_out.device) if nan_ops else program_tables(prog, x_out.device)
                tables = self._bound_tables[key]
                if nan_ops:
                    ops.bound_columns_(x_out, tables.ops, tables.params, nan_mask=nan_mask, n_nan_ops=tables.n_nan_ops)
                else:
                    ops.bound_columns_(x_out, *tables)
        return x_out

    def _extended_output_program(self, x_out: Tensor, ds: str, members: list, imputer, nan_mask: Optional[Tensor]) -> Tensor:
        """The boundings, then the inverse ops of every member of the post chain, last member first, as ONE in-place launch of the extended
        column program.  The imputer's NaN restoration is part of it when its mask was written by the input assembly (``nan_mask``); when the
        imputer ran stand-alone, ``forward`` restores after this (no post-processor stands before an imputer in a fusable chain)."""
        from ..layers.bounding import apply_program_torch, extended_program_tables
        from ..preprocessing import BaseImputer

        if torch.is_grad_enabled() and x_out.requires_grad:
            x_out = apply_program_torch(x_out, [op for b in self.boundings[ds] for op in b.program()])
            for member in reversed(members):
                if not (isinstance(member, BaseImputer) and nan_mask is None):
                    x_out = member.inverse_transform(x_out, in_place=False)
            return x_out
        if not x_out.is_contiguous():
            x_out = x_out.contiguous()
        # (built once per chain and normaliser state, as the tables of the plain program)
        state = tuple((id(m), m._norm_mul._version, m._norm_add._version) if hasattr(m, "_norm_mul") else (id(m),) for m in members)
        key = (ds, str(x_out.device), "ext", nan_mask is not None) + state
        if key not in self._bound_tables:
            width = x_out.shape[-1]
            prog = [op for b in self.boundings[ds] for op in b.program()]
            for member in reversed(members):
                if isinstance(member, BaseImputer) and nan_mask is None:
                    continue
                prog += member.inverse_program(width)
            self._bound_tables[key] = extended_program_tables(prog, width, x_out.device)
        tables = self._bound_tables[key]
        if tables[0].shape[0]:
            ops.column_program_(x_out, *tables, nan_mask=nan_mask)
        return x_out

    @scoped_forward
    def forward(self, x: dict, *, model_comm_group=None, grid_shard_sizes: Optional[dict] = None, _fused_norm: Optional[dict] = None,
                **kwargs) -> dict:
        """``_fused_norm`` (set by ``predict_step`` only): {dataset: (input normaliser, output normaliser[, imputer])} - x is then the RAW
        batch and the output is de-normalised; with an imputer, NaN of its variables is imputed on the way in and restored on the way out."""
        names = list(x.keys())
        batch_size = x[names[0]].shape[0]
        ensemble_size = x[names[0]].shape[2]
        if ensemble_size != 1:
            # the reference's class fails on it as well (node attributes are repeated batch_size times against batch * ensemble *
            # grid input rows: torch.cat mismatch at encoder_processor_decoder.py:121); its ensemble model folds members into the batch
            raise ValueError(f"AnemoiModelEncProcDec: ensemble dimension {ensemble_size} != 1; fold the members into the batch dimension")
        in_out_sharded = {ds: grid_shard_sizes is not None and grid_shard_sizes.get(ds) is not None for ds in names}
        if model_comm_group is not None and comm_size(model_comm_group) > 1:
            assert batch_size == 1, "Only batch size of 1 is supported when model is sharded across GPUs"
            assert ensemble_size == 1, "Ensemble size per device must be 1 when model is sharded across GPUs"
        hid = self._graph_name_hidden
        x_hidden_latent = self._hidden_attributes(batch_size)
        shard_sizes_hidden = get_shard_sizes(x_hidden_latent, 0, model_comm_group)
        x_hidden_latent = shard_tensor(x_hidden_latent, 0, shard_sizes_hidden, model_comm_group)
        latents, skips, data_latents, data_shards = {}, {}, {}, {}
        # one dataset, GraphTransformer on both sides: one carrier for the forward, so that the encoder's tail can hand the processor's first
        # block its projection (unsharded) and the last processor block's tail the decoder's block its k|v (layers/handoff.py)
        from ..layers.handoff import Carrier
        from ..layers.mapper import GraphTransformerBackwardMapper, GraphTransformerForwardMapper
        from ..layers.processor import GraphTransformerProcessor

        carrier = None
        if len(names) == 1 and isinstance(self.encoder[names[0]], GraphTransformerForwardMapper) and isinstance(self.processor, GraphTransformerProcessor):
            carrier = Carrier(next_block=self.processor.proc[0] if model_comm_group is None else None)
        chain_kw = {} if carrier is None else {"carrier": carrier}
        global LAST_SIDE_JOB_PANELS
        side_job = LAST_SIDE_JOB_PANELS = None
        if carrier is not None and model_comm_group is None and not torch.is_grad_enabled():
            carrier.static_dst = x_hidden_latent  # (inference: the cached static attribute tensor - the encoder may keep what it computes from it)
        for ds in names:
            shard_sizes_data = grid_shard_sizes[ds] if in_out_sharded[ds] else None
            norm_in, norm_out, *rest = (_fused_norm or {}).get(ds, (None, None))
            imputer, remapper, post_members = (tuple(rest) + (None, None, None))[:3]
            x_ds, ornstein_skip = x[ds], None
            if self._ornstein[ds]:
                # the Ornstein form acts on normalised values (predict_step does not fuse the normaliser for it).  The reference's residual
                # runs first and leaves its low-pass filtered fields in the model input (layers/residual.py:560-563 through
                # _assemble_input, models/encoder_processor_decoder.py:110-127): the encoder sees them, so it does here - on a copy
                assert norm_in is None, "SpectralOrnsteinConnection takes normalised inputs"
                res = self.residual[ds]
                x_ds = x_ds.clone() if res.truncate else x_ds
                ornstein_skip = res.compact(x_ds[:, -1], shard_sizes_data, write_back=res.truncate)
            x_data_latent, x_skip, raw, nan_mask, remap_fused = self._assemble_input(x_ds, batch_size, shard_sizes_data, model_comm_group, ds,
                                                                                     norm=norm_in, imputer=imputer, remapper=remapper)
            if nan_mask is not None:  # the nan_locations the imputer's own transform would have left; no loss mask at inference
                imputer.record_nan_locations(nan_mask.unsqueeze(0), nan_mask.shape[-1], loss_mask=False)
            if self._truncated[ds]:  # once per dataset and forward: down (columns, normaliser), up; the skip is then normalised
                x_skip = ornstein_skip if self._ornstein[ds] else self._truncated_skip(ds, x_skip, raw, norm_in, shard_sizes_data)
                raw = False
            skips[ds], data_shards[ds] = _EdgeState(x_skip, raw, norm_in, norm_out, imputer, nan_mask, remapper, remap_fused, post_members), shard_sizes_data
            if (_SIDE_JOB and carrier is not None and model_comm_group is None and not torch.is_grad_enabled()
                    and isinstance(self.decoder[ds], GraphTransformerBackwardMapper)):
                side_job = carrier.side_job = self.decoder[ds].destination_side_job(x_data_latent, _SIDE_PANELS_PER_RIDER)
            ea, ei, es = self.encoder_graph_provider[ds].get_edges(batch_size=batch_size, model_comm_group=model_comm_group)
            info = BipartiteGraphShardInfo(src_nodes=shard_sizes_data, dst_nodes=shard_sizes_hidden, edges=es)
            x_data_latent, x_latent = self.encoder[ds]((x_data_latent, x_hidden_latent.to(x_data_latent.dtype)), batch_size=batch_size,
                                                       shard_info=info, edge_attr=ea, edge_index=ei,
                                                       model_comm_group=model_comm_group, keep_x_dst_sharded=True, **chain_kw)
            data_latents[ds], latents[ds] = x_data_latent, x_latent
        x_latent = latents[names[0]] if len(names) == 1 else sum(latents.values())
        ea, ei, es = self.processor_graph_provider.get_edges(batch_size=batch_size, model_comm_group=model_comm_group)
        # the latent skip (:295-296) rides in the last processor block's last GEMM (GraphTransformer processor), else one add
        fuse_skip = self.latent_skip and isinstance(self.processor, GraphTransformerProcessor)
        # (GraphTransformer decoder, unsharded inference: the decoder block's layer_norm_attention_src + k|v projection of the hidden rows ride
        # at the end of the last processor block's chain launch, behind the latent skip)
        dec0 = self.decoder[names[0]]
        hand_kv = (_TAIL_KV and fuse_skip and carrier is not None and model_comm_group is None and isinstance(dec0, GraphTransformerBackwardMapper)
                   and not torch.is_grad_enabled())
        x_latent_proc = self.processor(x=x_latent, batch_size=batch_size, shard_info=GraphShardInfo(nodes=shard_sizes_hidden, edges=es),
                                       edge_attr=ea, edge_index=ei, model_comm_group=model_comm_group, **chain_kw,
                                       **({"latent_skip": x_latent} if fuse_skip else {}), **({"after_last_block": dec0.proc} if hand_kv else {}))
        if self.latent_skip and not fuse_skip:
            if (x_latent_proc.is_cuda and x_latent_proc.dim() == 2 and x_latent_proc.shape == x_latent.shape and x_latent_proc.dtype == x_latent.dtype
                    and not (torch.is_grad_enabled() and (x_latent_proc.requires_grad or x_latent.requires_grad))):
                from ..layers.block import _identity_index  # inference (GNN processor): the add as one launch of this library, not a torch kernel

                x_latent_proc = ops.gather_add_rows(x_latent_proc, x_latent, _identity_index(x_latent))
            else:
                x_latent_proc = x_latent_proc + x_latent
        out = {}
        for ds in names:
            ea, ei, es = self.decoder_graph_provider[ds].get_edges(batch_size=batch_size, model_comm_group=model_comm_group)
            info = BipartiteGraphShardInfo(src_nodes=shard_sizes_hidden, dst_nodes=data_shards[ds], edges=es)
            x_out = self.decoder[ds]((x_latent_proc, data_latents[ds]), batch_size=batch_size, shard_info=info, edge_attr=ea,
                                     edge_index=ei, model_comm_group=model_comm_group, keep_x_dst_sharded=in_out_sharded[ds], **chain_kw)
            if side_job is not None:
                LAST_SIDE_JOB_PANELS = (side_job.hosted, side_job.n_panels - side_job.hosted)
            e = skips[ds]
            out[ds] = self._assemble_output(x_out, e.x_skip, batch_size, ensemble_size, x[ds].dtype, ds, norm=e.norm_in, skip_is_raw=e.skip_is_raw,
                                            denorm=e.norm_out, compact=self._truncated[ds], imputer=e.imputer, nan_mask=e.nan_mask,
                                            remapper=e.remapper, remap_fused=e.remap_fused, post_members=e.post_members)
            if e.imputer is not None and e.nan_mask is None:  # imputed by the stand-alone kernel on the way in: restored by its counterpart
                out[ds] = e.imputer.inverse_transform(out[ds].contiguous(), in_place=True)  # (several output steps: a permuted clone)
        return out

    # -- predict_step (models/base.py:303-391) ----------------------------------------------------------------------------
    @staticmethod
    def _edge_chain(procs, inverse: bool):
        """(imputer or None, InputNormalizer) of a ``Processors`` chain the model edge can fuse - the normaliser alone, or one imputer followed
        by the normaliser (the members of an inverse chain are stored in the same order and applied last to first) - else None: two
        imputers, an imputer after the normaliser or a member of any other type stay opaque processors.

        A chain [imputer]? [Remapper]? InputNormalizer with post-processors (``Postprocessor`` family: the identity going forward) anywhere
        after the imputer fuses as well and comes back as (imputer or None, InputNormalizer, Remapper or None, members): ``members`` is the
        whole list in its stored order, from which the output column program takes every member's inverse ops, last member first.  A
        post-processor BEFORE the imputer would have to run after the NaN restoration, which a stand-alone imputer performs after the
        program: such a chain stays opaque, as does a Remapper after the normaliser."""
        from ..preprocessing import BaseImputer, InputNormalizer, Postprocessor, Processors, Remapper

        if isinstance(procs, InputNormalizer):
            return None, procs
        if not isinstance(procs, Processors) or procs.inverse != inverse:
            return None
        members = list(procs.processors.values())
        core = [m for m in members if not isinstance(m, Postprocessor)]
        if not core or not isinstance(core[-1], InputNormalizer):
            return None
        imputer = core[0] if isinstance(core[0], BaseImputer) else None
        rest = core[1:-1] if imputer is not None else core[:-1]
        if len(rest) > 1 or (rest and type(rest[0]) is not Remapper) or (imputer is not None and members[0] is not imputer):
            return None
        remapper = rest[0] if rest else None
        if remapper is None and len(core) == len(members):
            return imputer, core[-1]
        return imputer, core[-1], remapper, members

    def predict_step(self, batch: dict, pre_processors, post_processors, n_step_input: int, model_comm_group=None,
                     gather_out: bool = True, **kwargs) -> dict:
        """Pre-process, forward, post-process (reference models/base.py:303-391): ``batch[ds]`` is [batch, time, grid, vars] of
        RAW data.  When a dataset's pre- / post-processor chains are just the input normaliser, it is fused into the model
        edges: the transform runs inside the input assembly kernel (and on the skip connection inside the residual kernel),
        the inverse inside the output column program - no pass of its own over the data.  The chain [one imputer, input normaliser]
        (and the inverse chain over the same two modules) is fused likewise: the imputation program runs in the same kernels, the NaN mask
        of the first step is written by the input assembly and read by the output column program, and the imputer's ``nan_locations`` is
        what its own transform would have left.  A ``Remapper`` between the imputer and the normaliser and post-processors
        (``Postprocessor`` family) anywhere after the imputer fuse too (``_edge_chain``): the remap program follows the imputation program
        in the assembly kernels, and the output column program holds every member's inverse ops in inverse-chain order.  Any other chain
        goes through the modules."""
        from ..distributed.primitives import gather_tensor

        with torch.no_grad():
            names = list(batch.keys())
            for ds in names:
                assert len(batch[ds].shape) == 4, (
                    f"The {ds} input tensor has an incorrect shape: expected a 4-dimensional tensor, got {batch[ds].shape}!")
            x = {ds: batch[ds][:, 0:n_step_input, None, ...] for ds in names}  # dummy ensemble dimension as 3rd index
            grid_shard_sizes = None
            if model_comm_group is not None:
                grid_shard_sizes = {ds: get_shard_sizes(x[ds], -2, model_comm_group) for ds in names}
                x = {ds: shard_tensor(x[ds], -2, grid_shard_sizes[ds], model_comm_group) for ds in names}
            fused = {}
            for ds in names:
                pre, post = self._edge_chain(pre_processors[ds], False), self._edge_chain(post_processors[ds], True)
                same = pre is not None and post is not None and len(pre) == len(post) and pre[0] is post[0]
                if same and len(pre) == 4:  # a Remapper or post-processors: the same modules in the same order (the normalisers may be two)
                    same = len(pre[3]) == len(post[3]) and all(a is b or (a is pre[1] and b is post[1]) for a, b in zip(pre[3], post[3]))
                if same and x[ds].is_cuda and not self._ornstein[ds]:  # (the Ornstein residual acts on normalised values)
                    imputer, remapper, members = pre[0], (pre[2] if len(pre) == 4 else None), (post[3] if len(post) == 4 else None)
                    pre, post = pre[1], post[1]
                    fused[ds] = (pre, post) if imputer is None and members is None else (pre, post, imputer, remapper, members)
                    check = getattr(pre_processors[ds], "check_first_batch", None)
                    if check is not None and getattr(pre_processors[ds], "_awaiting_first_batch", False):
                        # the chain's one-off NaN check survives the fusion: the member modules run once, on a copy (with the remapper's
                        # domain assertion, which the fused kernels do not evaluate)
                        first = x[ds] if imputer is None else imputer.transform(x[ds], in_place=False)
                        if remapper is not None:
                            first = remapper.transform(first if first.stride(-1) == 1 else first.contiguous(), in_place=imputer is not None)
                        check(pre.transform(first, in_place=False))
                else:
                    x[ds] = pre_processors[ds](x[ds], in_place=False)
            y_hat = self.forward(x, model_comm_group=model_comm_group, grid_shard_sizes=grid_shard_sizes, _fused_norm=fused, **kwargs)
            for ds in names:
                if ds not in fused:
                    y_hat[ds] = post_processors[ds](y_hat[ds], in_place=False)
            if gather_out and model_comm_group is not None:
                for ds in names:
                    y_hat[ds] = gather_tensor(y_hat[ds], -2, grid_shard_sizes[ds], model_comm_group)
        return y_hat
