"""bench.py with ``CurlSacAgent(critic_layer_norm=True, critic_dropout=0.01)``: what the DroQ critic costs per update.

python tools/critic_dropout_bench.py [every bench.py option, e.g. --gpus 1 --steps 200 --warmup 20]

Runs bench.py's own ``main()`` -- its configurations, ring prefill, warm-up, timing and JSON line, unedited -- with the
one agent it builds constructed with both keywords (bench.py looks ``curla_amd.CurlSacAgent`` up when it builds the
agent; this wraps that name), as tools/critic_ln_bench.py does with the LayerNorm alone.  The JSON line is bench.py's,
so the figure compares with ``python bench.py`` (the default path) and ``python tools/critic_ln_bench.py`` (LayerNorm
only) of the same build directly; ``"critic_layer_norm": true, "critic_dropout": 0.01`` are added to it.  One GPU: the
wrapper is not carried into the ranks ``--gpus N`` would spawn."""
import functools
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

P = 0.01  # DroQ's


def main():
    import bench
    import curla_amd
    if "--gpus" in sys.argv and sys.argv[sys.argv.index("--gpus") + 1] != "1":
        sys.exit("tools/critic_dropout_bench.py measures one GPU")
    curla_amd.CurlSacAgent = functools.partial(curla_amd.CurlSacAgent, critic_layer_norm=True, critic_dropout=P)
    emit = bench.emit

    def tagged(obj):
        emit(dict(obj, critic_layer_norm=True, critic_dropout=P))
    bench.emit = tagged
    bench.main()


if __name__ == "__main__":
    main()
