"""Exponential moving average (EMA) of the weights: ``train.Engine(ema_decay=...)`` keeps one, ``engine.ema_weights()`` evaluates with it.

Semantics are timm's ``ModelEmaV2`` - a copy at construction, ``e += (1 - decay) * (p - e)`` after every optimizer step, buffers included -
with ``ModelEmaV3``'s optional warm-up ``decay_t = min(decay, (1 + n) / (10 + n))``.  Differences from timm: the average is one flat fp32
range plus a table of the module buffers instead of a second module; integer buffers (``num_batches_tracked``, the dropout seed) are not
averaged (timm copies them); an optimizer step that was skipped (fp16 overflow) does not update; ``every`` > 1 updates on every k-th
optimizer step with the SAME decay (timm has no such option).  The reference trains without an average (train.py:142,204-210,381-384).
All arithmetic is in csrc/ema.cpp; the counters live on the device, so the update is part of the captured step.
"""
import contextlib

import torch

from . import ops


class WeightEMA:
    """Averages ``arena.params[:active_numel]`` (under bf16 / fp16 storage: the fp32 master weights) and every floating-point module buffer.
    Frozen and never-reached parameters sit behind ``active_numel``, never change, and are their own average.  This object owns every buffer:
    ``flat`` (the arena range's average), ``buf_flat`` (the buffers' averages, back to back), ``state`` = [decay, num_updates, last_opt_step,
    coef] and the device pointer table of the buffer launch."""

    def __init__(self, model, arena, optimizer, decay, every=1, warmup=False):
        if not 0.0 < float(decay) < 1.0:
            raise ValueError("ema_decay must lie in (0, 1) (got %r); None = no average" % (decay,))
        if int(every) != every or every < 1:
            raise ValueError("ema_every must be an integer >= 1 (got %r)" % (every,))
        self.model, self.arena, self.optimizer = model, arena, optimizer
        self.decay, self.every, self.warmup = float(decay), int(every), bool(warmup)
        dev = arena.params.device
        self.n = arena.active_numel
        self.flat = torch.empty(self.n, dtype=torch.float32, device=dev)
        self.state = torch.zeros(4, dtype=torch.float32, device=dev)
        self.state[0] = self.decay
        self.buffers = []
        for name, b in model.named_buffers():
            if not b.is_floating_point() or b.numel() == 0:
                continue      # num_batches_tracked, the dropout seed: counters, not weights
            if b.dtype != torch.float32 or not b.is_contiguous() or b.device != dev:
                raise NotImplementedError("weight EMA: buffer %s is %s on %s (contiguous fp32 buffers on the model's device only)" % (name, b.dtype, b.device))
            self.buffers.append((name, b))
        total = sum(b.numel() for _, b in self.buffers)
        self.buf_flat = torch.empty(max(total, 1), dtype=torch.float32, device=dev)
        self.buf_views, off = [], 0
        for _, b in self.buffers:
            self.buf_views.append(self.buf_flat[off:off + b.numel()])
            off += b.numel()
        self._table, self._table_key = None, None
        self.swapped = False
        self.reset_from_live()
        self._buffer_table(check=True)      # built here, outside any capture; update() uses it as it stands
        self._named_views()                 # every averaged tensor must be found in model.state_dict(): fail at construction, not in a checkpoint

    # ---- the update (captured with the optimizer step)
    def _buffer_table(self, check=False):
        """The device table of the buffer launches.  ``check``: compare the live buffers' addresses with the table's and rebuild it when one
        was re-allocated (model.to(...)) - done at construction, in ``swap()`` and by ``invalidate()``, not on the step path."""
        if check:
            key = tuple(b.data_ptr() for _, b in self.buffers)
            if key != self._table_key:      # never while capturing (ops.ema_table asserts)
                self._table = ops.ema_table(zip(self.buf_views, (b for _, b in self.buffers))) if self.buffers else None
                self._table_key = key
        return self._table

    def invalidate(self):
        """Call after anything that re-allocated a module buffer: the pointer table is rebuilt (outside graph capture)."""
        self._buffer_table(check=True)

    def reset_from_live(self):
        """The average becomes a copy of the live values (timm's deep copy); the counters restart."""
        with torch.no_grad():
            self.flat.copy_(self.arena.params[:self.n])
            for v, (_, b) in zip(self.buf_views, self.buffers):
                v.copy_(b.reshape(-1))
            self.state.copy_(torch.tensor([self.decay, 0.0, 0.0, 0.0], dtype=torch.float32))

    def update(self):
        """Tick, the flat apply, the buffer-table apply: three launches behind the optimizer step (train.Engine._opt_step / _after_opt)."""
        if self.swapped:
            raise RuntimeError("weight EMA: update() while the averaged weights are swapped in (inside ema_weights())")
        table = self._buffer_table()
        ops.ema_tick_(self.state, self.optimizer.state, self.every, self.warmup)
        if self.n:
            ops.ema_apply_(self.flat, self.arena.params[:self.n], self.state)
        if table is not None:
            ops.ema_apply_multi_(table, self.state)

    @property
    def num_updates(self):
        return int(self.state[1])

    def tensors(self):
        """What a step mutates here (train.Engine._capture snapshots it around its warm-up steps)."""
        return [self.flat, self.buf_flat, self.state]

    # ---- swap
    def swap(self):
        """Exchanges live and averaged values in place: the arena range (every parameter is a view of it, so every module sees the change)
        and the float buffers; the 16-bit weight copies of the storage modes are rewritten from what is live now."""
        dev = self.arena.params.device
        if dev.type == "cuda" and torch.cuda.is_current_stream_capturing():
            raise RuntimeError("weight EMA: swap() while a stream is capturing")
        table = self._buffer_table(check=True)
        if self.n:
            ops.swap_(self.flat, self.arena.params[:self.n])
        if table is not None:
            ops.swap_multi_(table)
        self.swapped = not self.swapped
        if ops.lowp_storage():
            ops.lowp_refresh_weights()

    @contextlib.contextmanager
    def weights(self):
        """``with ema.weights():`` the model computes with the averaged values; they are swapped back on the way out, also on an exception."""
        if self.swapped:
            raise RuntimeError("weight EMA: ema_weights() is already active (it does not nest)")
        self.swap()
        try:
            yield self
        finally:
            self.swap()

    # ---- state, keyed by name in model.state_dict()'s layouts
    def _named_views(self):
        """{state_dict key: tensor of the average in the live tensor's shape and strides}, for the averaged entries of model.state_dict()."""
        by_ptr = {p.data_ptr(): (p, off) for _, p, off in self.arena.layout if off < self.n}
        bufs = {b.data_ptr(): (b, v) for (_, b), v in zip(self.buffers, self.buf_views)}
        out, sd = {}, self.model.state_dict()
        for k, t in sd.items():
            hit = by_ptr.get(t.data_ptr())
            if hit is not None and tuple(hit[0].shape) == tuple(t.shape) and t.is_floating_point():
                out[k] = torch.as_strided(self.flat, t.shape, t.stride(), self.flat.storage_offset() + hit[1])
            elif t.data_ptr() in bufs and t.is_floating_point():
                out[k] = bufs[t.data_ptr()][1].view(t.shape)
        got = {v.data_ptr() for v in out.values()}
        lost = [name for name, p, off in self.arena.layout if off < self.n and p.numel() and self.flat.data_ptr() + 4 * off not in got]
        lost += [name for (name, b), v in zip(self.buffers, self.buf_views) if name in sd and v.data_ptr() not in got]      # non-persistent buffers have no entry
        assert not lost, "weight EMA: %d averaged tensors were not matched to model.state_dict() entries (e.g. %s)" % (len(lost), lost[:3])
        return out

    def model_state_dict(self):
        """``model.state_dict()`` with the averaged values (clones): the average where there is one, the live value elsewhere (frozen and
        never-reached parameters, integer buffers)."""
        if self.swapped:
            raise RuntimeError("weight EMA: state_dict() inside ema_weights()")
        views = self._named_views()
        return {k: (views[k] if k in views else t).detach().clone() for k, t in self.model.state_dict().items()}

    def state_dict(self):
        st = self.state.tolist()
        return {"model": self.model_state_dict(), "num_updates": int(st[1]), "last_opt_step": int(st[2]), "decay": self.decay}

    def load_model_state_dict(self, sd):
        """Restores the average from a ``model.state_dict()``-shaped dict (``module.`` prefixes are stripped); entries without an average are ignored."""
        if self.swapped:
            raise RuntimeError("weight EMA: load_state_dict() inside ema_weights()")
        sd = {(k[len("module."):] if k.startswith("module.") else k): v for k, v in sd.items()}
        views = self._named_views()
        missing = [k for k in views if k not in sd]
        if missing:
            raise ValueError("weight EMA: the state has no entry for %d averaged tensors (e.g. %s)" % (len(missing), missing[:3]))
        with torch.no_grad():
            for k, v in views.items():
                v.copy_(sd[k])

    def load_counters(self, sd):
        self.state.copy_(torch.tensor([self.decay, float(sd["num_updates"]), float(sd["last_opt_step"]), 0.0], dtype=torch.float32))

    def load_state_dict(self, sd):
        self.load_model_state_dict(sd["model"])
        self.load_counters(sd)
