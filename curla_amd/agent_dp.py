"""CurlSacAgent's synchronous data parallelism: the gradient buckets' all-reduce and the check of the replicas."""
import os

import torch

from . import ops


class _DataParallelMixin:
    """CurlSacAgent's data-parallel methods; the ``_dp_*`` state they use is the agent's (CurlSacAgent.__init__)."""

    def enable_data_parallel(self, process_group=None, single_rank_collectives=False, overlap=None, broadcast=True,
                             check_every=None):
        """Synchronous data parallelism (one process per GPU): before every
        optimizer step the freshly written flat gradient bucket is averaged over
        ranks (RCCL over xGMI).  RCCL averages inside the collective
        (ncclAvg); other backends (gloo in the CPU tests) sum and divide.

        ``broadcast``: rank 0's parameters, targets and log_alpha replace every
        other rank's (three flat buffers + one scalar), so ranks need not have
        been seeded identically.  ``check_every`` (default 1000 updates, env
        CURLA_DP_CHECK_EVERY, 0 = never): a checksum of the replicated state is
        compared across ranks and a mismatch raises -- replicas that drift apart
        would otherwise train on silently.
        ``overlap`` (default off, env CURLA_DP_OVERLAP=1 turns it on): each
        bucket is reduced in two asynchronous pieces issued where their
        gradients become final -- the twin-Q / fc / LayerNorm gradients (almost
        all of the bytes) before the conv backward starts, the conv gradients
        after it -- on the communicator's own stream; the compute stream only
        waits for them right before ``optimizer.step()``.  Off: one blocking
        all-reduce per bucket.  Both orders reduce the same elements with the
        same collective, so the result does not depend on the flag.  The default
        follows the only measurement available so far (one GPU, one-rank RCCL
        group): the asynchronous schedule costs 0.12 ms per update more than the
        blocking one, like everything else that runs next to the persistent conv
        grids (DESIGN.md sections 6, 7); flip it once an N-GPU run says otherwise.
        ``single_rank_collectives`` issues the collectives even in a world of one
        (a 1-GPU check of the exact calls an N-GPU run makes)."""
        import torch.distributed as dist
        self._dp_group = process_group if process_group is not None else dist.group.WORLD
        self._dp_world = dist.get_world_size(self._dp_group)
        self._dp_active = self._dp_world > 1 or single_rank_collectives
        self._dp_avg = dist.get_backend(self._dp_group) == "nccl"
        # A backend without a device path of its own (gloo: the CPU tests, and the two-ranks-on-one-GPU test that RCCL
        # refuses) gets the buckets through the host: device -> host copy, collective, copy back, all synchronous.
        self._dp_staged = not self._dp_avg and self.device.type == "cuda"
        if overlap is None:
            overlap = os.environ.get("CURLA_DP_OVERLAP", "0") == "1"
        self._dp_overlap = bool(overlap)
        if check_every is None:
            check_every = int(os.environ.get("CURLA_DP_CHECK_EVERY", "1000"))
        self._dp_check_every = int(check_every)
        self._dp_pending = []
        if self._dp_active and broadcast:
            src = dist.get_global_rank(self._dp_group, 0)
            with torch.no_grad():
                for t in (self._critic_flat, self._target_flat, self._actor_flat, self.log_alpha):
                    if self._dp_staged:
                        h = t.detach().cpu()
                        dist.broadcast(h, src=src, group=self._dp_group)
                        t.copy_(h)
                    else:
                        dist.broadcast(t, src=src, group=self._dp_group)

    def _replica_checksum(self):
        """float64 sums of the replicated state (deterministic: same kernel, same data => same bits)."""
        with torch.no_grad():
            return torch.stack([self._critic_flat.sum(dtype=torch.float64), self._target_flat.sum(dtype=torch.float64),
                                self._actor_flat.sum(dtype=torch.float64), self.log_alpha.detach().to(torch.float64)])

    def _replica_check_due(self, step, first):
        """Whether a sub-step of update ``step`` checks the replicas: the call's ``first`` one, every ``check_every``."""
        return first and self._dp_active and self._dp_check_every > 0 and step % self._dp_check_every == 0

    def check_replicas(self):
        """Raise if the ranks' parameters differ (costs one 64-byte all-reduce and a host sync)."""
        if not self._dp_active:
            return
        import torch.distributed as dist
        s = self._replica_checksum()
        both = torch.stack([s, -s])  # max over ranks of (s, -s) = (max, -min)
        if self._dp_staged:
            both = both.cpu()
        dist.all_reduce(both, op=dist.ReduceOp.MAX, group=self._dp_group)
        hi, lo = both[0], -both[1]
        if not bool(torch.equal(hi, lo)):
            names = ("critic", "critic_target", "actor", "log_alpha")
            bad = [n for n, a, b in zip(names, hi.tolist(), lo.tolist()) if a != b]
            raise RuntimeError("data-parallel replicas have diverged (%s differ across ranks): seed every rank "
                               "identically or keep broadcast=True in enable_data_parallel" % ", ".join(bad))

    def _allreduce(self, *buckets, async_op=False, f64_rider=None):
        """Average each tensor over the ranks.  async_op: the collectives are only enqueued (they start once
        the compute stream reaches this point); _allreduce_wait() makes the compute stream wait for them.
        ``f64_rider`` = (scalar, words): ``scalar`` (one float64 element: log_alpha's gradient) rides in ``words``, the
        last ops.F64_WORDS elements of the LAST bucket -- packed before the collective, unpacked (= the mean over the
        ranks, from the exact sum: curla_hip.h curla_f64_pack) once it has completed."""
        if not self._dp_active:
            return
        import torch.distributed as dist
        if f64_rider is not None:
            scalar, words = f64_rider
            assert words.data_ptr() + 4 * words.numel() == buckets[-1].data_ptr() + 4 * buckets[-1].numel()
            ops.f64_pack(scalar, words)
        last = len(buckets) - 1
        for i, t in enumerate(buckets):
            if t.numel() == 0:
                continue
            avg = self._dp_avg and t.dtype == torch.float32  # (a float64 bucket of its own would take the sum path)
            op = dist.ReduceOp.AVG if avg else dist.ReduceOp.SUM
            post = []
            if not avg and not self._dp_staged:
                post.append(lambda t=t: t.div_(self._dp_world))
            if f64_rider is not None and i == last:
                # every path leaves the AVERAGED digits in the words: n_mul makes them the digit sums again
                post.append(lambda: ops.f64_unpack(f64_rider[1], self._dp_world, self._dp_world, f64_rider[0]))
            if self._dp_staged:  # (synchronous whatever async_op says: same elements, same sum)
                h = t.detach().cpu()
                dist.all_reduce(h, op=dist.ReduceOp.SUM, group=self._dp_group)
                t.copy_(h.div_(self._dp_world))
                work = None
            elif async_op:
                work = dist.all_reduce(t, op=op, group=self._dp_group, async_op=True)
            else:
                dist.all_reduce(t, op=op, group=self._dp_group)
                work = None
            if work is not None:
                self._dp_pending.append((work, post))
            else:
                for fn in post:
                    fn()

    def _allreduce_wait(self):
        for work, post in self._dp_pending:
            work.wait()
            for fn in post:
                fn()
        self._dp_pending = []

    def _grad_offset(self, p, flat):
        return (p.grad.data_ptr() - flat.data_ptr()) // 4
