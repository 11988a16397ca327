"""The statistics plumbing of the engines as dataflow: on the recording backend (tests/trace_ops.py, no arithmetic) every forward
of the trace matrix must read only statistics that an earlier launch of the same forward wrote, and reduce no partial buffer
twice.  Properties only - whether two trees run the same schedule is what tools/schedule_trace.py is diffed for.

NOT asserted yet: "every chan_parts / row_parts buffer that is written is read afterwards".  The present schedule does not have
that property in 12 of the 40 cases - the producers below are asked for sums that nobody takes - and changing what a producer is
asked for changes the launch sequence, which belongs in a change of its own together with this assertion:
  * every DIRECT_STATS row of (2, 4, 32, 32) and (4, 2, 16, 16) and the temb_first row: 2 chan_parts buffers per forward.  The
    last layer of an up block that ends in an upsampler is asked for the sums of a clip-level norm, but its output goes into
    the upsampling convolution alone.  With the fold off the same two buffers are reduced at once and the reduced sums are
    never read: two chan_stats_reduce launches per forward in the default configuration.
  * the fused-kernel DIRECT_STATS rows of (2, 2, 12, 8): 1 buffer.  The upsampling convolution writes sums for the two-source
    norm1 of the next layer, whose skip connection has none (fyc_ff_block at 96-row frames): the norm takes the concat and
    the statistics pass.
  * FUSE_ROWS with the fused kernels: 36 row_parts buffers in front of fyc_ff_block / fyc_temporal_block, which normalise in
    registers."""
import pytest

import trace_ops
from trace_ops import buffers, written

# arguments through which a launch reads statistics of an activation
STAT_READS = dict(gn_apply_cs=("cs1", "cs2", "parts1", "parts2"), panel_linear=("gn_cs", "gn_parts"), gemm=("ln_stats",),
                  chan_stats_reduce=("parts",))


def check(log):
    assert log
    produced, reduced = set(), set()
    for i, l in enumerate(log):
        for name in STAT_READS.get(l.op, ()):
            for b in buffers(l.args.get(name)):
                assert b.storage in produced, f"launch {i} ({l.op}) reads {name} = storage {b.storage}, which no earlier launch wrote"
        if l.op == "chan_stats_reduce":
            s = l.args["parts"].storage
            assert s not in reduced, f"launch {i} reduces storage {s} a second time"
            reduced.add(s)
        produced.update(b.storage for b in written(l))


@pytest.mark.parametrize("case", trace_ops.unet_cases(), ids=lambda c: c[0])
def test_unet_statistics_dataflow(case):
    log = trace_ops.run_unet(case).log
    check(log)
    if not case[2].get("DIRECT_STATS", False):      # no consumer takes raw partials, every reduce sits right behind its producer
        assert not any(l.args.get("parts1") or l.args.get("parts2") or l.args.get("gn_parts") for l in log)
        for i, l in enumerate(log):
            if l.op == "chan_stats_reduce":
                assert l.args["parts"] in list(buffers([log[i - 1].args.get("chan_parts")])), i


@pytest.mark.parametrize("case", trace_ops.vae_cases(), ids=lambda c: c[0])
def test_vae_statistics_dataflow(case):
    log = trace_ops.run_vae(case).log
    check(log)
    assert any(l.op == "chan_stats_reduce" for l in log) == case[3]      # FYC_VAE_FUSE_STATS
