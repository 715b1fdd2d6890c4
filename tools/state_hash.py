"""sha256 over the state an agent is in after 12 updates: what "bit-identical to the parent commit" is checked with.

python tools/state_hash.py [--bins0] [--gaussian] [--infonce]

Builds tests/test_gpu_utd._build(1)'s agent and buffer (B = 256, hidden 64, LayerNorm + dropout critics), runs
update() for steps 1..12 and hashes, key by key in sorted order, everything tests/test_gpu_utd._state collects: the flat
parameters of critic, target and actor, the Adam moments and step counts, log_alpha, and the torch (device and CPU) and
NumPy random streams.  ``--bins0`` passes ``critic_bins=0``, ``--gaussian`` ``policy="gaussian"`` and ``--infonce``
``cpc_objective="infonce"``; without them no keyword is passed, so the same file runs on a checkout from before the keywords.  Run it from the root of each checkout and compare the lines."""
import hashlib
import os
import sys

sys.path.insert(0, os.getcwd())

from tests.test_gpu_critic_ln import NullLogger  # noqa: E402
from tests.test_gpu_utd import _build, _state  # noqa: E402


def main():
    hp = dict(critic_bins=0) if "--bins0" in sys.argv[1:] else {}
    if "--gaussian" in sys.argv[1:]:
        hp["policy"] = "gaussian"
    if "--infonce" in sys.argv[1:]:
        hp["cpc_objective"] = "infonce"
    agent, rb, _ = _build(1, hp=hp)
    L = NullLogger()
    for step in range(1, 13):
        agent.update(rb, L, step)
    state = _state(agent, rb)
    h = hashlib.sha256()
    for k in sorted(state):
        h.update(k.encode())
        h.update(state[k].contiguous().numpy().tobytes())
    print("STATE", ", ".join("%s=%s" % kv for kv in sorted(hp.items())) or "no keyword", h.hexdigest())


if __name__ == "__main__":
    main()
