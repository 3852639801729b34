"""Training engine: one process per GPU, data-parallel over utterances with RCCL.

The reference trains on a single device through ``tf.estimator`` (``asr/train.py:31-55``,
``train_distribute=None``); the step it runs is forward -> CTC loss -> backward -> Adam
(``asr/model.py:49-83``).  `Trainer.train_step` is that step written out over the HIP kernels,
plus what BASELINE.json adds: minibatches sharded across the GPUs of a node, gradients summed
with RCCL all-reduce over xGMI — per layer slice of the flat gradient arena, launched as soon
as the backward pass has finished that layer so the collective overlaps the rest of backward.
"""

import collections
import types
import warnings
import os
import time

import torch
import torch.distributed as dist

from ctc_asr_amd import params as _params
from ctc_asr_amd.model import CTCModel


def init_distributed(backend=None):
    """Initialise ``torch.distributed`` from the torchrun environment (RANK / LOCAL_RANK /
    WORLD_SIZE / MASTER_*).  Returns (rank, local_rank, world_size).  ``backend`` defaults to
    'nccl' (= RCCL on ROCm) when a GPU is visible, else 'gloo'."""
    world = int(os.environ.get('WORLD_SIZE', '1'))
    rank = int(os.environ.get('RANK', '0'))
    local_rank = int(os.environ.get('LOCAL_RANK', '0'))
    if world > 1 and not dist.is_initialized():
        os.environ.setdefault('MASTER_ADDR', '127.0.0.1')
        os.environ.setdefault('MASTER_PORT', '29500')
        os.environ.setdefault('HSA_ENABLE_IPC_MODE_LEGACY', '0')
        if backend is None:
            backend = os.environ.get('CTCASR_DIST_BACKEND') or \
                ('nccl' if torch.cuda.is_available() else 'gloo')
        if backend == 'nccl':
            torch.cuda.set_device(local_rank)
        dist.init_process_group(backend=backend, rank=rank, world_size=world)
    return rank, local_rank, world


class NanLossDuringTrainingError(RuntimeError, FloatingPointError):
    """The training loss is NaN or infinite: what the reference's ``NanTensorHook`` raises
    (``asr/model.py:368``; ``tf.train.NanLossDuringTrainingError`` is a RuntimeError).  Raised by
    the deferred checks of `Trainer` (the guard word of the step that hit it, at most
    `max_steps_ahead` steps later) and by `train.train_epoch` where it reads the loss."""


class GradientReducer:
    """Bucketed sum-all-reduce of the flat gradient arena.

    ``hook(layer, start, stop)`` is called by ``CTCModel.backward`` when a layer's slice is
    final; slices are merged into buckets of at least ``bucket_bytes`` (contiguous because the
    arena is laid out in layer order and backward walks it from the end) and each bucket is
    reduced asynchronously.  ``finish()`` flushes the remainder and waits.  With world size 1
    everything is a no-op.  xGMI is point-to-point (7 links x ~153 GB/s per GPU): buckets of
    tens of MB keep each ring step bandwidth- rather than latency-bound without delaying the
    first launch."""

    def __init__(self, grad_arena, world_size, bucket_bytes=64 << 20, group=None,
                 hold_until=None, force=False, max_bucket_bytes=None, stand_in=None):
        self.grad, self.world, self.group = grad_arena, world_size, group
        # ``stand_in`` = (workgroups, GB/s): instead of a collective every bucket launches a
        # kernel of that many resident workgroups that holds its CUs for bytes / rate on a
        # stream of its own - ordered after the launching stream and waited for by `finish()`
        # exactly like an asynchronous all-reduce.  The one-GPU stand-in for RCCL's ring kernels
        # beside the persistent recurrences (NCCL refuses two ranks on one device); implies
        # `force`.  Gradients are left alone (a one-rank sum).
        self.stand_in = stand_in
        self._stand_in_stream = None
        self._stand_in_scratch = None
        # `force`: run the collectives even with a single rank (a world-size-1 process group is
        # legal): tests use it to put the real backend (RCCL) under the real backward pass on a
        # one-GPU box
        self.active = world_size > 1 or force or stand_in is not None
        self.bucket_elems = max(1, bucket_bytes // 4)
        # slices are merged until a bucket holds at least `bucket_bytes`; a pending range larger
        # than `max_bucket_bytes` (a held-back release: everything at once; or one big layer) is
        # cut into equal pieces no larger than that, so that the first piece's ring steps start
        # while the later ones are still being enqueued and no single collective is hundreds of MB
        self.max_bucket_elems = max(self.bucket_elems,
                                    (max_bucket_bytes or max(bucket_bytes, 64 << 20)) // 4)
        self.pending_start = None
        self.pending_stop = None
        self.works = []
        self.launched = 0               # all-reduce launches so far (bench.py reports per step)
        # Collective kernels must not be in flight while a persistent recurrence kernel starts:
        # that kernel needs all of its workgroups co-resident (one per CU) and spins at grid
        # barriers, so RCCL workgroups holding CUs could stall it past its spin limit.  With
        # `hold_until` = name of the last recurrent layer of the backward pass, buckets are only
        # launched from that layer's hook on - they then overlap the remaining weight-gradient
        # GEMMs and the conv backward, which have no residency requirement.
        self.hold_until = hold_until
        self.released = hold_until is None

    def __call__(self, layer, start, stop):
        self.hook(layer, start, stop)

    def flush(self):
        """Launch whatever is pending now (if released).  `CTCModel.backward` calls this at the
        end of the block of hooks that run with the side stream current: those slices were
        produced by side-stream GEMMs, so their all-reduce must be enqueued while that stream is
        still the current one - never merged into a bucket that is launched later from the main
        stream, which is not ordered after them."""
        if self.active and self.released:
            self._flush()

    def hook(self, layer, start, stop):
        if not self.active:
            return
        if layer == self.hold_until:
            self.released = True
        if self.pending_stop is None:
            self.pending_start, self.pending_stop = start, stop
        else:
            # backward visits layers from the end of the arena towards its start
            if stop != self.pending_start:       # not adjacent: cannot merge into one view
                self._flush()
                self.pending_start, self.pending_stop = start, stop
            else:
                self.pending_start = start
        if self.released and self.pending_stop - self.pending_start >= self.bucket_elems:
            self._flush()

    def _flush(self):
        if self.pending_stop is None:
            return
        start, stop = self.pending_start, self.pending_stop
        pieces = -(-(stop - start) // self.max_bucket_elems)
        piece = -(-(stop - start) // pieces)
        piece = (piece + 3) // 4 * 4                 # keep 16-byte alignment of every view
        hi = stop
        while hi > start:                            # from the end: the order backward made them
            lo = max(start, hi - piece)
            if self.stand_in is not None:
                self.works.append(self._launch_stand_in((hi - lo) * 4))
            else:
                self.works.append(dist.all_reduce(self.grad[lo:hi], op=dist.ReduceOp.SUM,
                                                  group=self.group, async_op=True))
            self.launched += 1
            hi = lo
        self.pending_start = self.pending_stop = None

    def _launch_stand_in(self, nbytes):
        """The stream semantics of `dist.all_reduce(async_op=True)` on the nccl backend: the
        collective runs on the backend's own stream behind everything enqueued so far on the
        launching stream; `wait()` makes the then-current stream wait for it."""
        from ctc_asr_amd import hip
        workgroups, gb_per_s = self.stand_in[:2]
        traffic = len(self.stand_in) > 2 and bool(self.stand_in[2])
        device = self.grad.device
        if traffic and self._stand_in_scratch is None:
            # (zeros: a += b stays zero however often it runs)
            self._stand_in_scratch = tuple(torch.zeros(16 << 20, dtype=torch.float32,
                                                       device=device) for _ in range(2))
        if self._stand_in_stream is None:
            self._stand_in_stream = torch.cuda.Stream(device)
        ready = torch.cuda.Event()
        ready.record(torch.cuda.current_stream(device))
        with torch.cuda.stream(self._stand_in_stream):
            self._stand_in_stream.wait_event(ready)
            busy_us = max(1, int(nbytes / (gb_per_s * 1e3)))
            if traffic:
                hip.collective_traffic(self._stand_in_scratch[0], self._stand_in_scratch[1],
                                       workgroups, busy_us, nbytes)
            else:
                hip.occupy_cus(workgroups, busy_us)
            done = torch.cuda.Event()
            done.record(self._stand_in_stream)

        class _Work:
            @staticmethod
            def wait():
                torch.cuda.current_stream(device).wait_event(done)
        return _Work

    def finish(self, guard=None):
        """Flush and wait.  ``guard`` (the int32 words of `CTCModel.step_guard`): with more than
        one rank its MAXIMUM over ranks comes back in place - a step that one replica must not
        apply carries that replica's gradients in every rank's sum, so every replica drops it
        (the Adam kernel's skip flag) and the parameters stay replicated until the error the
        bad rank raises stops the job."""
        if not self.active:
            return
        self.released = self.hold_until is None
        self._flush()
        if guard is not None and self.world > 1 and self.stand_in is None:
            self.works.append(dist.all_reduce(guard, op=dist.ReduceOp.MAX, group=self.group,
                                              async_op=True))
        for work in self.works:
            work.wait()
        self.works = []


class Trainer:
    """Owns a `CTCModel` replica on this rank's GPU and runs synchronous data-parallel steps."""

    def __init__(self, cfg, flags=None, device=None, seed=0, params=None, world_size=1, rank=0,
                 bucket_bytes=64 << 20, conv_autotune=None, allreduce_early=None,
                 force_reducer=False, reduce=True, collective_stand_in=None, max_grad_norm=None,
                 report_grad_norms=None, grad_accum_steps=None, ema_decay=None, lr_schedule=None,
                 mwer_nbest=None, mwer_beam_width=None, mwer_ctc_weight=None, mwer_risk=None):
        self.world, self.rank = world_size, rank

        def flag(name, default):
            return getattr(flags, name, default) if flags is not None else default

        # Minimum word error rate training (keyword arguments, else the flags of the same names,
        # else off): with ``mwer_nbest`` >= 2 a step's loss is the expected error count over the
        # n-best list of its own logits plus ``mwer_ctc_weight`` times the CTC loss
        # (`CTCModel.mwer_loss_fn`); each rank decodes its own shard.  With 0 `train_step`
        # launches exactly what it launches without it.
        mwer = {'nbest': int(flag('mwer_nbest', 0) if mwer_nbest is None else mwer_nbest)}
        for name, given in (('beam_width', mwer_beam_width), ('ctc_weight', mwer_ctc_weight),
                            ('risk', mwer_risk)):
            default = _params.MWER_DEFAULTS['mwer_' + name]
            mwer[name] = flag('mwer_' + name, default) if given is None else given
        _params.check_mwer_settings(**mwer)
        self.mwer = mwer if mwer['nbest'] else None
        self.last_expected_risk = None  # device float32[B]: R_b of the last (micro-)step
        self.last_mwer_paths = None     # device int32[B]: the sizes of its lists

        # The schedule of a run (keyword arguments, else the flags of the same names, else off):
        # ``grad_accum_steps`` micro-batches are summed into one update, ``ema_decay`` > 0 keeps
        # an exponential moving average of the parameters in the Adam launch, ``lr_schedule`` /
        # --lr_warmup_steps move the learning rate with the update count.  With all three off
        # `train_step` launches exactly what it launches without them.
        self.grad_accum_steps = int(flag('grad_accum_steps', 1) if grad_accum_steps is None
                                    else grad_accum_steps)
        if not 1 <= self.grad_accum_steps <= 1024:
            raise ValueError('grad_accum_steps={} is outside 1..1024.'.format(
                self.grad_accum_steps))
        self.ema_decay = float(flag('ema_decay', 0.0) if ema_decay is None else ema_decay)
        if not 0.0 <= self.ema_decay < 1.0:
            raise ValueError('ema_decay={} is outside 0 <= d < 1.'.format(self.ema_decay))
        self.lr_schedule = str(flag('lr_schedule', 'constant') if lr_schedule is None
                               else lr_schedule)
        if self.lr_schedule not in _params.LR_SCHEDULES:
            raise ValueError('lr_schedule={} is none of {}.'.format(
                self.lr_schedule, ', '.join(_params.LR_SCHEDULES)))
        self._micro = 0                 # micro-steps of the open update that have run
        self._accum_guard = None        # ... and their guard words, or-ed, on the device
        # Clipping by global norm (``max_grad_norm`` > 0) and the per-layer norms
        # (``report_grad_norms``): keyword arguments, else the flags of the same names, else off.
        # With both off `train_step` launches exactly what it launches without them.
        if max_grad_norm is None:
            max_grad_norm = getattr(flags, 'max_grad_norm', 0.0) if flags is not None else 0.0
        if report_grad_norms is None:
            report_grad_norms = getattr(flags, 'report_grad_norms', False) \
                if flags is not None else False
        self.max_grad_norm = float(max_grad_norm)
        self.report_grad_norms = bool(report_grad_norms)
        self.last_grad_norms = None     # device float32: per layer (`CTCModel.grad_norm_names`)
        self.last_clip_factor = None    # ... then the global norm; device float32[1]
        self._clipped = None
        device = device or 'cuda:{}'.format(torch.cuda.current_device())
        self.model = CTCModel(cfg, device, seed=seed, params=params, conv_autotune=conv_autotune,
                              ema=self.ema_decay > 0)
        self.lr = getattr(flags, 'learning_rate', 1e-5) if flags is not None else 1e-5
        # what `params.learning_rate_at` reads; under 'constant' without warm-up `self.lr` is left
        # alone (it is the flag's value already, and callers may set it)
        defaults = _params.FLAGS.defaults_dict()
        self._lr_flags = types.SimpleNamespace(
            learning_rate=self.lr, lr_schedule=self.lr_schedule,
            **{name: flag(name, defaults[name])
               for name in ('learning_rate_decay_factor', 'steps_per_decay', 'minimum_lr',
                            'lr_warmup_steps', 'lr_total_steps')})
        self.lr_scheduled = self.lr_schedule != 'constant' or self._lr_flags.lr_warmup_steps > 0
        if self.lr_scheduled:
            _params.learning_rate_at(1, self._lr_flags)     # (refuses an incomplete schedule now)
        self.beta1 = getattr(flags, 'adam_beta1', 0.9) if flags is not None else 0.9
        self.beta2 = getattr(flags, 'adam_beta2', 0.999) if flags is not None else 0.999
        self.eps = getattr(flags, 'adam_epsilon', 1e-8) if flags is not None else 1e-8
        # Release of the gradient buckets (``allreduce_early``; None = CTCASR_ALLREDUCE_EARLY):
        #   early (default since round 6)
        #                   every layer's bucket is reduced as soon as its weight-gradient GEMMs
        #                   are done on the side stream, beside the recurrences of the layers
        #                   below.  RCCL's workgroups occupy CUs for as long as a collective runs;
        #                   the H = 1024 backward recurrence needs 128 of the 256 CUs, so both
        #                   fit - a persistent workgroup that finds its CU taken waits (spin
        #                   limit: seconds).
        #   held            nothing is reduced before the last persistent recurrence launch of
        #                   the backward pass has been issued (`hold_until='rnn0'`).
        # Why early: with a stand-in that has a ring all-reduce's CU footprint AND its memory
        # traffic beside the real step (one GPU) the C3 step pays +2.3 ms
        # (4.6 %) for early against +5.3 ms (10.4 %) for held, and neither mode timed out; held
        # leaves the whole 0.49 GB of gradients to be reduced behind the backward pass.  bench.py
        # measures both modes at N > 1 and reports the better one, so a node on which RCCL beside
        # the recurrences behaves worse than the stand-in still shows in the line.
        # Models whose recurrence takes ALL 256 CUs (LSTM / GRU at H = 2048) always hold: there
        # the hooks run on the main stream right in front of whole-chip persistent launches,
        # whose resident workgroups would spin until the collective has drained.
        if allreduce_early is None:
            allreduce_early = os.environ.get('CTCASR_ALLREDUCE_EARLY', '1') == '1'
        whole_chip = cfg.cell in ('lstm', 'gru') and cfg.num_units_rnn == 2048
        early = bool(allreduce_early) and not whole_chip
        active = (world_size > 1 or force_reducer or collective_stand_in is not None) and reduce
        self.model.early_hooks = early and active
        # ``reduce=False`` (bench.py's "stubbed" leg): the same step without any collective, to
        # price what the all-reduce adds to it; replicas drift apart - timing only
        self.reducer = GradientReducer(self.model.arena.grad, world_size if reduce else 1,
                                       bucket_bytes, hold_until=None if early else 'rnn0',
                                       force=force_reducer and reduce,
                                       stand_in=collective_stand_in if reduce else None)
        self.release = 'early' if early else 'held'
        if world_size > 1:   # identical replicas: rank 0's initial parameters win
            dist.broadcast(self.model.arena.param, src=0)
            self.model.arena.touch()
            self.model.arena.seed_ema()
        # The host enqueues a step several times faster than the GPU runs it.  Left alone it
        # runs ahead without bound: every step's activations (5 GB at C3) are then allocated
        # anew - blocks freed by the host are still in use by steps the GPU has not reached -
        # until the allocator hits the end of HBM and synchronises.  `max_steps_ahead` bounds
        # the lead: step N is not enqueued before step N - max_steps_ahead has finished.
        self.max_steps_ahead = 2
        self._step_done = collections.deque()
        self.host_wait_s = 0.0          # time spent waiting there (bench.py reports the rest)
        # Deferred error checks (``train_step(check=True)``): a step's CTC status words travel to
        # pinned host memory with an asynchronous copy and are looked at when that step is known
        # to have finished - at the wait above, `max_steps_ahead` steps later - and the sticky
        # time-out word of the persistent recurrence kernels (no launch clears it) is polled
        # every `rnn_poll_every` steps and by `drain_checks()`.  Neither stalls the host, so the
        # run-ahead above also holds for real training, not only for the benchmark.
        self.rnn_poll_every = 50
        self._pending_status = collections.deque()
        self._skipped = None
        self._skipped_reconciled = 0
        self._steps_since_poll = 0

    def _check_finished_steps(self, wait=False):
        """Raise for any finished step whose CTC status reported an infeasible alignment /
        bad labels (``wait``: block until every pending step has finished)."""
        while self._pending_status:
            event, host, step, norm_host = self._pending_status[0]
            if not wait and not event.query():
                break
            event.synchronize()
            self._pending_status.popleft()
            words = host.numpy()
            try:
                CTCModel.check_status(host[:-2])
            except ValueError as err:
                raise type(err)('{} [training step {}; its update was not applied]'.format(
                    err, step)) from None   # (``step``: "7", or "7 (micro-step 1 of 2)")
            if words[-1] != 0:
                # a persistent recurrence gave up at a grid barrier in that step: the sticky word
                # is read (and the barrier words reset) by the synchronous poll, which raises
                self.model.check_rnn_error()
            if words[-2] != 0:
                raise NanLossDuringTrainingError(
                    'NaN loss during training. [non-finite CTC loss in training step {}; its '
                    'update was not applied]'.format(step))
            if norm_host is not None and not torch.isfinite(norm_host).all():
                # a finite loss whose gradients hold an inf or a NaN: `ctcasr_grad_norm` raised the
                # guard word itself
                raise NanLossDuringTrainingError(
                    'Non-finite gradients during training. [non-finite gradient norm in training '
                    'step {}; its update was not applied]'.format(step))

    def drain_checks(self):
        """Wait for the steps in flight and raise what they have to report: CTC status of every
        pending step, then the persistent kernels' time-out word.  `train.train_epoch` calls
        this where it reads the loss anyway, at the end of an epoch and before a checkpoint.
        Refuses inside an open update (`accumulating`): its micro-steps' gradients are in the
        arena and no step has been counted for them."""
        self._refuse_open_update('drain_checks')
        self._check_finished_steps(wait=True)
        self.model.check_rnn_error()
        self._steps_since_poll = 0
        # Steps the device dropped without a check having raised for them (`train_step(check=
        # False)`, --no-step-checks): TensorFlow's global step would not have advanced - take them
        # back out of the step counter here, where the host is synchronised anyway, so that Adam's
        # bias correction and the step a checkpoint is written under count applied updates only
        # (ADVICE r05), and say so.
        dropped = self.skipped_step_count()
        if dropped > self._skipped_reconciled:
            new = dropped - self._skipped_reconciled
            self._skipped_reconciled = dropped
            self.model.step_count -= new
            warnings.warn('{} training step(s) were dropped on the device (CTC status, non-finite '
                          'loss or gradient norm, or a kernel time-out); the step counter is back '
                          'at {}.'.format(new, self.model.step_count), RuntimeWarning)

    @property
    def accumulating(self):
        """True while an update is open: some, not all, of its ``grad_accum_steps`` micro-steps
        have run."""
        return self._micro > 0

    def _refuse_open_update(self, what):
        if self.accumulating:
            raise RuntimeError('{}: update {} is open ({} of {} micro-steps have run); finish it '
                               'or `abandon_update()` first.'.format(
                                   what, self.model.step_count + 1, self._micro,
                                   self.grad_accum_steps))

    def abandon_update(self):
        """Drop the open update, if any: the gradients its micro-steps left in the arena are
        cleared by the next one's first backward pass, nothing was counted.  What
        `train.train_epoch` does with a ragged last group.  The micro-steps' deferred checks
        stay queued."""
        self._micro, self._accum_guard = 0, None

    def save_checkpoint(self, train_dir, epoch, extra=None):
        """`storage.save_checkpoint` of this trainer's model; refuses inside an open update."""
        from ctc_asr_amd import storage
        self._refuse_open_update('save_checkpoint')
        return storage.save_checkpoint(train_dir, self.model, epoch, extra)

    def train_step(self, features, feature_len, labels, check=True, originals=None):
        """forward + CTC + backward (+ all-reduce) + Adam on this rank's shard of the global
        batch; returns the local mean loss (device scalar).  The global loss is the mean over
        ranks of the local means (equal shard sizes), so gradients are summed and scaled by
        1 / world_size inside the Adam kernel.

        ``originals``: the transcripts of the batch, read only by MWER training with the word
        risk (``mwer_nbest`` >= 2; default: the labels decoded).  The loss is then the expected
        error count plus the weighted CTC loss, and `last_expected_risk` holds the former.

        ``check=True``: errors are raised without stalling the host - an infeasible alignment
        (where ``tf.nn.ctc_loss`` raises), a non-finite loss or a timed-out persistent kernel
        surfaces at most `max_steps_ahead` steps after the step that hit it (the guard word
        travels to pinned memory with the CTC status), and always before a checkpoint is
        written; with `max_grad_norm` / `report_grad_norms` on, so does a gradient norm that is
        not finite behind a finite loss.  Either way that step's update is dropped ON THE DEVICE
        (`CTCModel.step_guard` -> the Adam kernel's skip flag): parameters and moments never see
        its gradients.

        ``grad_accum_steps`` = k > 1: a call is one MICRO-step.  The first k - 1 of an update run
        forward + backward into the gradient arena (the first clears it, the others add), or
        their guard words into one kept on the device and return; the k-th also runs the reducer
        hooks, the norms and Adam, on the summed arena with 1 / (world * k).  One raised guard
        word in any of them drops the whole update.  `model.step_count` counts updates."""
        if len(self._step_done) >= self.max_steps_ahead:
            t0 = time.perf_counter()
            while len(self._step_done) >= self.max_steps_ahead:
                self._step_done.popleft().synchronize()
            self.host_wait_s += time.perf_counter() - t0
        if check:
            self._check_finished_steps()
            self._steps_since_poll += 1
            if self._steps_since_poll >= self.rnn_poll_every:
                # (synchronises: once per `rnn_poll_every` steps)
                self._check_finished_steps(wait=True)
                self.model.check_rnn_error()
                self._steps_since_poll = 0
        accum = self.grad_accum_steps
        last = self._micro == accum - 1
        label = self.model.step_count + 1
        # (off: the calls below are the calls of a trainer that knows nothing of MWER)
        extra = {'mwer': self.mwer, 'originals': originals} if self.mwer else {}
        if accum > 1:
            label = '{} (micro-step {} of {})'.format(label, self._micro + 1, accum)
            loss = self.model.forward_backward(features, feature_len, labels,
                                               reduce_hook=self.reducer if last else None,
                                               check=False, accumulate=self._micro > 0, **extra)
        else:
            loss = self.model.forward_backward(features, feature_len, labels,
                                               reduce_hook=self.reducer, check=False, **extra)
        if self.mwer:
            self.last_expected_risk = self.model.last_mwer['expected_risk']
            self.last_mwer_paths = self.model.last_mwer['n_hyps']
        # Invalid gradients never reach the parameters: the guard word is computed on the device
        # from this step's CTC status, its loss and the recurrence time-out words, and the Adam
        # kernel drops the update when it is set - whenever the host gets to look.
        # (N > 1: the guard words are max-reduced with the gradients, every replica drops the
        # step that one of them must not apply; the rank that hit it raises.)
        guard = self.model.step_guard()
        norms_on = self.max_grad_norm > 0 or self.report_grad_norms
        if check:
            status = self.model.last_status
            host = torch.empty(status.numel() + 2, dtype=status.dtype, pin_memory=True)
            host[:status.numel()].copy_(status, non_blocking=True)
            host[status.numel():].copy_(guard, non_blocking=True)
            if not norms_on or not last:
                copied = torch.cuda.Event()
                copied.record(torch.cuda.current_stream(self.model.device))
                self._pending_status.append((copied, host, label, None))
        if accum > 1:
            # (the host copy above holds this micro-step's own words: its check names it)
            if self._accum_guard is not None:
                guard |= self._accum_guard
            if not last:
                self._accum_guard = guard
                self._micro += 1
                done = torch.cuda.Event()
                done.record(torch.cuda.current_stream(self.model.device))
                self._step_done.append(done)
                return loss
            self._micro, self._accum_guard = 0, None
        grad_scale = 1.0 / self.world if accum == 1 else 1.0 / (self.world * accum)
        self.reducer.finish(guard)      # (N > 1: the guard words become their maxima over ranks)
        grad_factor = None
        if norms_on:
            # AFTER the all-reduce, on the summed gradients: every rank then reads bit-identical
            # values, the kernel's summation order is fixed, so every rank computes the identical
            # norm and the identical factor (and raises the guard word on the same steps) - the
            # replicas stay replicated without another collective.  1 / world: the norm of the
            # MEAN gradient, what Adam applies.  Nothing comes back to the host here: the factor
            # stays on the device and the Adam kernel reads it.
            norms, grad_factor = self.model.grad_norms(grad_scale, self.max_grad_norm, guard)
            self.last_grad_norms, self.last_clip_factor = norms, grad_factor
            if self._clipped is None:
                self._clipped = torch.zeros(1, dtype=torch.int32, device=self.model.device)
            # (a factor of 0 is a dropped step - `skipped_step_count()` - not a clipped one)
            self._clipped += ((grad_factor > 0) & (grad_factor < 1)).to(torch.int32)
            if check:
                norm_host = torch.empty(1, dtype=torch.float32, pin_memory=True)
                norm_host.copy_(norms[-1:], non_blocking=True)
                copied = torch.cuda.Event()
                copied.record(torch.cuda.current_stream(self.model.device))
                self._pending_status.append((copied, host, label, norm_host))
        # (how many updates the device has dropped so far: `skipped_step_count()` - a run whose
        # steps were silently skipped must not be reported as throughput)
        if self._skipped is None:
            self._skipped = torch.zeros(1, dtype=torch.int32, device=self.model.device)
        self._skipped += (guard[:1] != 0).to(torch.int32)
        if self.lr_scheduled:
            self.lr = _params.learning_rate_at(self.model.step_count + 1, self._lr_flags)
        if self.ema_decay > 0:
            self.model.apply_gradients(self.lr, self.beta1, self.beta2, self.eps,
                                       grad_scale=grad_scale, skip=guard,
                                       grad_factor=grad_factor, ema_decay=self.ema_decay)
        else:
            self.model.apply_gradients(self.lr, self.beta1, self.beta2, self.eps,
                                       grad_scale=grad_scale, skip=guard,
                                       grad_factor=grad_factor)
        done = torch.cuda.Event()
        done.record(torch.cuda.current_stream(self.model.device))
        self._step_done.append(done)
        return loss

    def skipped_step_count(self):
        """Training steps whose update the device dropped (guard word set: CTC status, non-finite
        loss, recurrence / weight-gradient time-out) since this trainer was built; synchronises.
        The step counter advances for such a step at first (TensorFlow's global step would not);
        `drain_checks()` takes it back out.  A dropped step always raises at the next check of
        `train_step(check=True)` / `drain_checks()`."""
        return 0 if self._skipped is None else int(self._skipped.item())

    def clipped_step_count(self):
        """Training steps whose gradients were scaled down to `max_grad_norm` (clip factor below
        1; a step dropped for a non-finite norm counts as skipped, not clipped) since this trainer
        was built; synchronises."""
        return 0 if self._clipped is None else int(self._clipped.item())

    def global_mean(self, value):
        """Average a device scalar over ranks (logged loss, eval metrics)."""
        if self.world <= 1:
            return value
        value = value.detach().clone()
        dist.all_reduce(value, op=dist.ReduceOp.SUM)
        return value / self.world
