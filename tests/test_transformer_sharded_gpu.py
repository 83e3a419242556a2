"""The heads-sharded TransformerProcessor (reference attention.py:190-227: local rows x all heads -> all rows x H / P heads -> attention ->
back) on 2 ranks sharing the one GPU (the spawn pattern and host transport of tests/test_distributed_gpu.py): equal to the unsharded
processor within the fp32 bound of tests/test_fullsize_parity_gpu._check; num_heads % P != 0 and batch_size != 1 raise."""
import pytest
import torch

from tests.test_distributed_gpu import _spawn
from tests.test_fullsize_parity_gpu import _check

pytestmark = pytest.mark.gpu
CASES = {
    "window8": dict(num_channels=64, num_heads=2, window_size=8),
    "alibi_softcap": dict(num_channels=128, num_heads=4, window_size=40, use_alibi_slopes=True, softcap=20.0),
    "qk_norm": dict(num_channels=128, num_heads=2, window_size=None, qk_norm=True),
}
SIZES = [330, 312]  # the two ranks' rows of a 642-row mesh


def _sharded_worker(rank, world, group, name):
    from anemoi_core_amd.distributed.shapes import GraphShardInfo
    from tests import transformer_helpers as T

    kw = CASES[name]
    proc = T.processor(kw).eval()
    T.fill(proc, 21)
    proc = proc.to("cuda")
    x = T.inputs(22, sum(SIZES), kw["num_channels"]).cuda()
    r0 = sum(SIZES[:rank])
    with torch.no_grad():
        full = proc(x, 1, GraphShardInfo(nodes=None))
        part = proc(x[r0:r0 + SIZES[rank]].contiguous(), 1, GraphShardInfo(nodes=SIZES), model_comm_group=group)
    return dict(full=full[r0:r0 + SIZES[rank]].cpu(), part=part.cpu())


@pytest.mark.parametrize("name", sorted(CASES))
def test_heads_sharded_processor_equals_unsharded(name):
    for o in _spawn(_sharded_worker, 2, name):
        _check(f"sharded transformer {name}", o["part"], o["full"], torch.float32)


def _raising_worker(rank, world, group):
    from anemoi_core_amd.distributed.shapes import GraphShardInfo
    from tests import transformer_helpers as T

    out = {}
    for label, kw, batch in (("heads", dict(num_channels=96, num_heads=3, window_size=8), 1),
                             ("batch", dict(num_channels=64, num_heads=2, window_size=8), 2)):
        proc = T.processor(kw).eval().cuda()
        x = torch.zeros(batch * SIZES[rank], kw["num_channels"], device="cuda")
        try:
            with torch.no_grad():
                proc(x, batch, GraphShardInfo(nodes=[batch * n for n in SIZES]), model_comm_group=group)
            out[label] = None
        except ValueError as e:
            out[label] = str(e)
    return out


def test_heads_not_divisible_by_ranks_and_batches_raise():
    for o in _spawn(_raising_worker, 2):
        assert o["heads"] is not None and "divisible" in o["heads"]
        assert o["batch"] is not None and "batch size of 1" in o["batch"]
