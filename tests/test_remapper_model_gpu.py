"""``AnemoiModelEncProcDec.predict_step`` with a Remapper and post-processors in the chain on the MI355X: fused into the model-edge kernels
(one sample, one output step), through the stand-alone kernels where the fused ones do not apply, and captured in a hipGraph - against the
reference's recorded predict_step (tests/golden/remapper.pt; the tiny model is that of tests/golden/edges.pt).  Two chains:
[ConditionalZero, Remapper, InputNormalizer, NormalizedRelu] and [InputImputer, Remapper, InputNormalizer] on a NaN-carrying batch.  The
model-level bounds are those of tests/test_imputer_model_gpu.py."""
from types import SimpleNamespace

import pytest
import torch

from anemoi_core_amd import ops
from anemoi_core_amd.preprocessing import InputImputer, InputNormalizer, Processors, Remapper
from tests.helpers import indices_from_fixture, model_config
from tests.model_edge_refs import assert_bits_equal
from tests.remapper_helpers import chain_members

pytestmark = pytest.mark.gpu
DEV = "cuda"
REL = 2e-5  # fp32, fused or through the modules, against the reference (tests/test_imputer_model_gpu.py, tests/test_edges_gpu.py)


class _Opaque(torch.nn.Module):
    """Hides a Processors chain from the fusion (as in tests/test_edges_gpu.py): the member modules run."""

    def __init__(self, inner):
        super().__init__()
        self.inner = inner

    def forward(self, x, **kw):
        return self.inner(x, **kw)


def _setup(golden, chain="post", dtype=torch.float32, n_step_output=1):
    from anemoi_core_amd.graphs.synthetic import build_synthetic_graph
    from anemoi_core_amd.models import AnemoiModelEncProcDec

    c, f = golden("edges.pt")["predict_step"], golden("remapper.pt")["predict_step"]
    cfg = c["cfg"]
    g = build_synthetic_graph(cfg["data_grid"], cfg["hidden_resolution"])
    di = indices_from_fixture(c["indices"])
    stats = {k: v.numpy().copy() for k, v in c["statistics"].items()}
    torch.manual_seed(0)
    model = AnemoiModelEncProcDec(model_config=model_config(cfg["kind"], cfg["num_channels"], cfg["num_layers"], cfg["num_heads"], cfg["trainable"]),
                                  data_indices={"data": di}, statistics={"data": stats}, n_step_input=cfg["n_step_input"],
                                  n_step_output=n_step_output, graph_data=g).eval()
    if n_step_output == 1:
        model.load_state_dict(c["params"], strict=True)
    norm_cfg = c["data_config"]["normalizer"]
    if chain == "post":
        members = chain_members(di, stats, f["remap_config"], norm_cfg, f["relu_config"], f["zero_config"])
        batch, out = c["batch"], f["out"]
    else:
        members = [["imputer", InputImputer(f["imputer_config"], di, stats)], ["remapper", Remapper(f["remap_config"], di, stats)],
                   ["normalizer", InputNormalizer(norm_cfg, di, stats)]]
        batch, out = f["imputer_batch"], f["imputer_out"]
    for _, m in members:
        m.to(DEV)
    return SimpleNamespace(model=model.to(DEV).to(dtype), members=members, pre=Processors(members), post=Processors(members, inverse=True),
                           n=cfg["n_step_input"], batch=batch, out=out)


def _step(s, batch, pre=None, post=None):
    return s.model.predict_step({"data": batch}, {"data": s.pre if pre is None else pre}, {"data": s.post if post is None else post}, s.n)["data"]


def _close(got, want, rel, what):
    """NaN at the same places; the finite rest within rel * max(1, max |want|)."""
    got, want = got.float().cpu(), want.float().cpu()
    assert got.shape == want.shape and torch.equal(got.isnan(), want.isnan()), f"{what}: NaN at other places"
    fin = ~want.isnan()
    scale = max(1.0, float(want[fin].abs().max()))
    err = float((got[fin] - want[fin]).abs().max())
    print(f"{what}: max error {err:.3e} at scale {scale:.3f} (bound {rel * scale:.3e})")
    assert err <= rel * scale, what


def _boom(what):
    def boom(*a, **k):
        raise AssertionError(f"{what} ran inside the fused predict_step")

    return boom


@pytest.mark.parametrize("chain", ["post", "imputer"])
def test_fused_predict_step_equals_reference_and_modules(golden, monkeypatch, chain):
    """Fused == the reference's recorded output == the same chain forced through the modules; the fused call launches no stand-alone kernel
    of the imputer, the remapper or the normaliser, and hands the remap program to both assembly kernels; the batch is untouched."""
    s = _setup(golden, chain)
    assert s.model._edge_chain(s.pre, False) is not None and len(s.model._edge_chain(s.pre, False)) == 4
    batch = s.batch.to(DEV)
    unfused = _step(s, batch, _Opaque(s.pre), _Opaque(s.post))
    _step(s, batch)  # (the chain's first-batch check runs the member modules once)
    for name in ("impute_columns", "restore_nan_columns", "affine_columns", "remap_columns"):
        monkeypatch.setattr(ops, name, _boom(f"ops.{name}"))
    seen = []
    real_in, real_out = ops.assemble_input, ops.assemble_output
    monkeypatch.setattr(ops, "assemble_input", lambda *a, **k: (seen.append(("in", k.get("remap") is not None, k.get("impute") is not None)), real_in(*a, **k))[1])
    monkeypatch.setattr(ops, "assemble_output", lambda *a, **k: (seen.append(("out", k.get("remap") is not None, k.get("impute") is not None)), real_out(*a, **k))[1])
    fused = _step(s, batch)
    assert seen == [("in", True, chain == "imputer"), ("out", True, chain == "imputer")]
    assert fused.dtype == torch.float32 and (chain == "post" or int(s.out.isnan().sum()) > 0)
    _close(fused, s.out, REL, "fused vs the reference")
    _close(unfused, s.out, REL, "modules vs the reference")
    _close(fused, unfused, REL, "fused vs modules")
    assert_bits_equal(batch, s.batch, "the batch")
    if chain == "post":  # the conditional fill acted: exact zeros of the remapper's inverse in v3 became 2.5, and v0 / v5 their values there
        assert int((fused[..., 3] == 2.5).sum()) == int((s.out[..., 3] == 2.5).sum()) > 0


def test_first_batch_check_keeps_the_domain_assertion(golden):
    """The fused kernels evaluate no assertion; the chain's one-off check runs the Remapper module on a copy, with it."""
    s = _setup(golden, "post")
    members = [["remapper", Remapper({"default": "none", "sqrt": ["v0"]}, s.members[1][1].data_indices, None)], s.members[2]]
    batch = s.batch.clone()
    batch[0, 0, 5, 0] = -1.0
    with pytest.raises(AssertionError, match="Power transform input x must satisfy x >= 0"):
        _step(s, batch.to(DEV), Processors(members), Processors(members, inverse=True))


@pytest.mark.parametrize("chain", ["post", "imputer"])
def test_fused_predict_step_replays_from_a_graph(golden, chain):
    """predict_step captured in a hipGraph (no host synchronisation once the first batch is checked): the replay equals the eager call bit
    for bit, also after the static input buffer was rewritten."""
    s = _setup(golden, chain)
    static = s.batch.to(DEV).clone()
    step = lambda: _step(s, static)  # noqa: E731
    for _ in range(2):
        first = step().clone()
    stream = torch.cuda.Stream()
    stream.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(stream):
        step()
    torch.cuda.current_stream().wait_stream(stream)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        out = step()
    graph.replay()
    torch.cuda.synchronize()
    assert_bits_equal(out, first.cpu(), "replay on the captured input")
    moved = s.batch.roll(5, dims=2).contiguous()
    static.copy_(moved.to(DEV))
    graph.replay()
    torch.cuda.synchronize()
    replayed = out.clone()
    assert_bits_equal(replayed, _step(s, moved.to(DEV)).cpu(), "replay on the rewritten input")
    assert not torch.equal(replayed.nan_to_num(0.0), first.nan_to_num(0.0))


@pytest.mark.parametrize("chain", ["post", "imputer"])
def test_batch_of_two_takes_the_stand_alone_kernels(golden, monkeypatch, chain):
    """Batch 2: the stand-alone kernels first, then the chain of the normaliser alone; the output program still holds the remapper's inverse
    and the post-processors.  The samples do not interact and sample 0 meets the reference."""
    s = _setup(golden, chain)
    b0 = s.batch.to(DEV)
    b1 = b0.roll(3, dims=2).contiguous()
    one = [_step(s, b) for b in (b0, b1)]
    seen = []
    real = ops.assemble_input
    monkeypatch.setattr(ops, "assemble_input", lambda *a, **k: (seen.append(k.get("remap") is not None), real(*a, **k))[1])
    two = _step(s, torch.cat([b0, b1], 0))
    assert not any(seen), "the remap program reached the fused assembly with a batch of two"
    assert two.shape[0] == 2
    for i in range(2):
        _close(two[i:i + 1], one[i], REL, f"sample {i}")
    _close(one[0], s.out, REL, "sample 0 vs the reference")


def test_two_output_steps_take_the_stand_alone_kernels(golden, monkeypatch):
    """Two output steps (a model of its own, seeded weights): the fusable chain and the same chain behind an opaque wrapper agree."""
    s = _setup(golden, "post", n_step_output=2)
    batch = s.batch.to(DEV)
    want = _step(s, batch, _Opaque(s.pre), _Opaque(s.post))
    seen = []
    real = ops.assemble_input
    monkeypatch.setattr(ops, "assemble_input", lambda *a, **k: (seen.append(k.get("remap") is not None), real(*a, **k))[1])
    got = _step(s, batch)
    assert not any(seen) and got.shape == want.shape and got.shape[1] == 2
    _close(got, want, REL, "two output steps: chain vs modules")


def test_bf16_model_on_fp32_data(golden):
    """fp32 data into a bf16 model: the 8-column route of the fused input assembly.  The bounds of tests/test_edges_gpu.py for this model in
    bf16, against the reference and against the modules."""
    s = _setup(golden, "imputer", torch.bfloat16)
    batch = s.batch.to(DEV)
    unfused = _step(s, batch, _Opaque(s.pre), _Opaque(s.post))
    out = _step(s, batch)
    assert out.dtype == torch.float32 and out.shape == s.out.shape
    assert torch.equal(out.isnan().cpu(), s.out.isnan()) and torch.equal(out.isnan(), unfused.isnan())
    fin = ~s.out.isnan()
    scale = max(1.0, float(s.out[fin].abs().max()))
    for what, ref in (("reference", s.out), ("modules", unfused.cpu())):
        err = (out.cpu()[fin] - ref[fin]).abs()
        print(f"bf16 vs {what}: max {float(err.max()):.3e}, mean {float(err.mean()):.3e}, scale {scale:.3f}")
        assert float(err.max()) <= 6e-2 * scale and float(err.mean()) <= 1e-2 * scale


@pytest.mark.parametrize("order", ["remapper_after_normalizer", "post_before_imputer"])
def test_chains_that_are_not_fused_give_the_module_result(golden, monkeypatch, order):
    """A Remapper after the normaliser and a post-processor in front of an imputer: predict_step runs the modules (the remap program never
    reaches the fused assembly) and returns, bit for bit, what the same chains give when an opaque wrapper hides them."""
    s = _setup(golden, "imputer")
    (_, imp), (_, rm), (_, nm) = s.members
    if order == "remapper_after_normalizer":
        di = rm.data_indices
        members = [["imputer", imp], ["normalizer", nm], ["remapper", Remapper({"default": "none", "asinh": ["v0"]}, di, None)]]
    else:
        zero = _setup(golden, "post").members[0]
        members = [zero, ["imputer", imp], ["remapper", rm], ["normalizer", nm]]
    pre, post = Processors(members), Processors(members, inverse=True)
    assert s.model._edge_chain(pre, False) is None
    batch = s.batch.to(DEV)
    want = _step(s, batch, _Opaque(pre), _Opaque(post))
    seen = []
    real = ops.assemble_input
    monkeypatch.setattr(ops, "assemble_input", lambda *a, **k: (seen.append(k.get("remap") is not None), real(*a, **k))[1])
    got = _step(s, batch, pre, post)
    assert seen and not any(seen)
    assert_bits_equal(got, want.cpu(), order)
