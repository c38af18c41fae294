"""``mx.mod.Module`` over the HIP executor (main_train.py:89-94,143-146; lib/inference.py:71-74,423-428).

Data parallelism is MI355X-native: one process per GPU.  Under ``torchrun`` (WORLD_SIZE > 1) every
rank binds its LOCAL_RANK device, consumes its slice ``batch[rank*B:(rank+1)*B]`` of the iterator's
global batch (the split MNIteratorBase.n_per_gpu implies, lib/iterators/MNIteratorBase.py:21) and the
gradient arena is summed with one RCCL all-reduce per step -- the only exchange the reference's
kvstore='device' performs.  A single process asked for several contexts is refused: that is the
reference's in-process multi-GPU model, which this engine deliberately does not have.
"""
import logging
import os
import time
from collections import namedtuple

import numpy as np
import torch

from . import ndarray as nd
from .misc import save_checkpoint

BatchEndParam = namedtuple('BatchEndParams', ['epoch', 'nbatch', 'eval_metric', 'locals'])


def _dist():
    import torch.distributed as dist
    if dist.is_available() and dist.is_initialized():
        return dist
    return None


def init_distributed():
    """Join the torchrun rendezvous (RCCL backend) if launched with WORLD_SIZE > 1."""
    import torch.distributed as dist
    ws = int(os.environ.get('WORLD_SIZE', '1'))
    if ws > 1 and not dist.is_initialized():
        torch.cuda.set_device(int(os.environ.get('LOCAL_RANK', '0')) % torch.cuda.device_count())
        dist.init_process_group(backend=os.environ.get('SNIPER_DIST_BACKEND', 'nccl'))
    return dist if ws > 1 else None


class Module(object):
    def __init__(self, symbol, data_names=('data',), label_names=('softmax_label',), logger=logging, context=None,
                 work_load_list=None, fixed_param_names=None, state_names=None):
        self.symbol = symbol
        self.data_names = list(data_names or [])
        self.label_names = list(label_names or [])
        self.logger = logger
        ctx = context if isinstance(context, (list, tuple)) else [context or nd.gpu(0)]
        self.contexts = list(ctx)
        self.fixed_param_names = list(fixed_param_names or [])
        self.binded = self.params_initialized = self.optimizer_initialized = False
        self.exe = None
        self._arg_params = self._aux_params = None
        self.world = int(os.environ.get('WORLD_SIZE', '1'))
        self.rank = int(os.environ.get('RANK', '0'))
        # True: the iterator yields the GLOBAL batch and every rank takes its slice (reference behaviour);
        # False: the iterator is already rank-local (bench.py: each rank owns an independent chip minibatch)
        self.slice_inputs = True
        self.static_loss_scale = None      # a static loss scale folded into lr / wd by the caller: only the monitor's 'loss_scale' row reads it

    # ---- properties the reference reads
    @property
    def output_names(self):
        return self.symbol.list_outputs()

    @property
    def data_shapes(self):
        return self._data_shapes

    @property
    def label_shapes(self):
        return self._label_shapes

    # ---- bind
    def _local(self, shape):
        """per-GPU shape of a batch-major input (global batch split across ranks / contexts)"""
        n = self.world if (self.world > 1 and self.slice_inputs) else 1
        if self.world == 1 and len(self.contexts) > 1:
            raise NotImplementedError(
                'one process driving %d GPUs is the reference\'s in-process model; launch one process per GPU instead: '
                'python -m torch.distributed.run --nproc-per-node %d ... (see INTEGRATION.md)' % (len(self.contexts),
                                                                                                len(self.contexts)))
        shape = tuple(shape)
        if n > 1:
            assert shape[0] % n == 0, 'batch %d not divisible by %d ranks' % (shape[0], n)
            return (shape[0] // n,) + shape[1:]
        return shape

    def bind(self, data_shapes, label_shapes=None, for_training=True, inputs_need_grad=False, force_rebind=False,
             shared_module=None, grad_req='write'):
        from ..engine.executor import Executor
        if self.binded and not force_rebind:
            return
        if self.world > 1:
            init_distributed()
        from ..engine.executor import thaw_heap
        thaw_heap()                  # (Modules dropped since the last settle_heap: their memory goes now)
        self.for_training = for_training
        self._data_shapes = [(d[0], tuple(d[1])) for d in data_shapes]
        self._label_shapes = [(d[0], tuple(d[1])) for d in (label_shapes or [])]
        shapes = {}
        for name, shp in self._data_shapes + self._label_shapes:
            shapes[name] = self._local(shp)
        args = set(self.symbol.list_arguments())
        shapes = {k: v for k, v in shapes.items() if k in args}
        # one process per GPU: rank-local device.  (Modulo the device count only matters for the single-GPU rehearsal of
        # the multi-rank control flow, SNIPER_DIST_BACKEND=gloo; a real launch has one device per local rank.)
        dev = torch.device('cuda', int(os.environ.get('LOCAL_RANK', self.contexts[0].device_id)) % torch.cuda.device_count()
                           if self.world > 1 else self.contexts[0].device_id)
        torch.cuda.set_device(dev)
        from .. import hip
        hip.use_device(dev.index)
        self._device = dev
        self._exes = {}          # test-time batches change shape (scale, chip size): one bound executor per input shape
        self.exe = self._exe_for(shapes)
        self.binded = True

    def _exe_for(self, shapes):
        from ..engine.executor import Executor
        key = tuple(sorted((k, tuple(v)) for k, v in shapes.items()))
        ex = self._exes.get(key)
        if ex is not None and not self.for_training:
            self._exes[key] = self._exes.pop(key)          # most recently used last
        if ex is None:
            # data parallel: backward in two segments, the first segment's gradients are all-reduced under the second
            ov = os.environ.get('SNIPER_OVERLAP_ALLREDUCE', '1')
            split = self.for_training and ((self.world > 1 and ov != '0') or ov == 'force')
            pool = None
            if not self.for_training and os.environ.get('SNIPER_SHARE_ACTIVATIONS', '1') != '0':
                from ..engine.executor import ActivationPool
                pool = self.__dict__.setdefault('_act_pool', None) or ActivationPool(self._device)
                self._act_pool = pool
            share = None
            if not self.for_training and self._exes and os.environ.get('SNIPER_SHARE_PARAMS', '1') != '0':
                share = next(iter(self._exes.values()))          # any bound shape: they all hold the Module's one parameter set
            ex = Executor(self.symbol, dict(shapes), for_training=self.for_training, fixed_param_names=self.fixed_param_names,
                          device=self._device, split_backward=split, act_pool=pool, share_params=share)
            if self._arg_params is not None:
                if share is not None and ex.adopt_derived():
                    # parameters AND everything derived from them are the Module's: nothing to do -- and nothing one-off left for a first,
                    # eager forward to settle, so this shape's FIRST forward is already the capture (engine/executor.py forward)
                    ex.capture_first = os.environ.get('SNIPER_CAPTURE_FIRST', '1') != '0'
                elif share is not None and all(n in ex.shared_names for n in list(ex.params) + list(ex.aux)):
                    ex.refresh_compute_copies()                  # the values are there: only this shape's derived buffers
                else:
                    ex.set_params(self._arg_params, self._aux_params)
            self._guard_exe(ex)
            self._accum_exe(ex)
            self._exes[key] = ex
            if not self.for_training:
                self._evict_stale(keep=ex)
                from ..engine.executor import settle_heap
                settle_heap()
        return ex

    def _evict_stale(self, keep=None):
        """Test-time executors are kept per (bucketed) batch shape, least recently used first out.  A pass over many images
        walks its area-sorted chip shapes in the same order every time, so a small first-in-first-out cache misses on EVERY
        batch once a scale has one shape more than it holds (64 images: 9 executors rebuilt per pass, 1.9 s instead of 0.3 --
        profiles/r04_infer_long_pass.txt).  The bound is memory, not a count: shapes are dropped only while this process holds
        more than SNIPER_EXE_CACHE_FRAC (default 0.6) of the card's HBM, or beyond SNIPER_EXE_CACHE executors (default 256)."""
        cap = int(os.environ.get('SNIPER_EXE_CACHE', '256'))
        frac = float(os.environ.get('SNIPER_EXE_CACHE_FRAC', '0.6'))
        total = 0
        if self._device.type == 'cuda':
            try:                          # (the runtime's own query: torch's device table can disagree with it under a
                total = torch.cuda.mem_get_info(self._device)[1]      # CUDA_VISIBLE_DEVICES it does not parse, main_test.py)
            except Exception:             # noqa: BLE001 -- no figure: the count bound alone
                total = 0

        def over():
            if len(self._exes) > cap:
                return True
            return bool(total) and torch.cuda.memory_allocated(self._device) > frac * total
        current, dropped = getattr(self, 'exe', None), False
        rotated = 0
        while len(self._exes) > 1 and over() and rotated < len(self._exes):
            key = next(iter(self._exes))
            if self._exes[key] is current or self._exes[key] is keep:
                # never the executor in use nor the one just built (`keep`, about to become self.exe): to the back of the queue
                self._exes[key] = self._exes.pop(key)
                rotated += 1
                continue
            self._exes.pop(key)
            live = set(kv for k in self._exes for kv in k)                 # (input name, shape) pairs some bound executor still takes
            for bk in [b for b in getattr(self, '_bucket_bufs', {}) if (b[0], tuple(b[1])) not in live]:
                del self._bucket_bufs[bk]              # the dropped shape's zero-padded input buffers (69 MB each at 1408 x 2048) go with it
            dropped = True
            import gc
            gc.unfreeze()                                  # (engine/executor.py::settle_heap put the executors out of the collector's reach)
            gc.collect()                                   # steps and executor reference each other: the tensors go with the cycle
        return dropped

    # ---- parameters
    def init_params(self, initializer=None, arg_params=None, aux_params=None, allow_missing=False, force_init=False,
                    allow_extra=True):
        if self.params_initialized and not force_init:
            return
        arg = dict(arg_params or {})
        aux = dict(aux_params or {})
        rs = np.random.RandomState(0)
        for name, p in self.exe.params.items():
            if name not in arg:
                if not allow_missing and arg_params is not None and initializer is None:
                    raise RuntimeError('%s is not presented' % name)
                if name.endswith('_gamma'):
                    arg[name] = np.ones(p.ref_shape, np.float32)
                elif name.endswith('_weight') and len(p.ref_shape) > 1:
                    fan_in = float(np.prod(p.ref_shape[1:]))
                    arg[name] = (rs.standard_normal(p.ref_shape) * np.sqrt(2.0 / fan_in)).astype(np.float32)  # MSRA
                else:
                    arg[name] = np.zeros(p.ref_shape, np.float32)
        for name, t in self.exe.aux.items():
            if name not in aux:
                aux[name] = np.ones(tuple(t.shape), np.float32) if name.endswith('_var') else np.zeros(tuple(t.shape), np.float32)
        self._arg_params = {k: (v.asnumpy() if hasattr(v, 'asnumpy') else np.asarray(v)) for k, v in arg.items()}
        self._aux_params = {k: (v.asnumpy() if hasattr(v, 'asnumpy') else np.asarray(v)) for k, v in aux.items()}
        for ex in self._exes.values():
            ex.set_params(self._arg_params, self._aux_params)
        self._broadcast_params()
        self.params_initialized = True

    def _broadcast_params(self):
        """Data parallel: every replica starts from rank 0's parameters (what kvstore.init + pull does in the reference's
        Module) -- mx.random / np.random draws of the head initialisers differ between processes otherwise."""
        d = _dist()
        if d is None or d.get_world_size() == 1:
            return
        for ex in self._exes.values():
            d.broadcast(ex.arena_master, src=0)
            for p in ex.params.values():          # frozen parameters live outside the arena (Executor._alloc_params): a randomly
                if not p.trainable:               # initialised frozen weight (synthetic runs, names missing from the pretrained
                    d.broadcast(p.master, src=0)  # file) must be the same on every replica too, as kvstore init + pull makes it
            for t in ex.aux.values():
                d.broadcast(t, src=0)
            ex.refresh_compute_copies()
        arg, aux = self.exe.get_params()
        self._arg_params, self._aux_params = arg, aux

    def set_params(self, arg_params, aux_params, allow_missing=False, force_init=True, allow_extra=True):
        self.init_params(None, arg_params, aux_params, allow_missing, force_init)

    def get_params(self):
        arg, aux = self.exe.get_params()
        return {k: nd.NDArray(v) for k, v in arg.items()}, {k: nd.NDArray(v) for k, v in aux.items()}

    def save_checkpoint(self, prefix, epoch, save_optimizer_states=False):
        if self.rank != 0:
            return
        if save_optimizer_states and getattr(self, '_accum_pending', 0) > 0:
            self.logger.warning('gradient accumulation: %d of %d micro-batches are pending; their gradients are not in the .states file, '
                                'a resumed run starts a new window', self._accum_pending, self.opt['accumulate'])
        arg, aux = self.get_params()
        save_checkpoint(prefix, epoch, self.symbol, arg, aux)
        if save_optimizer_states:
            states = {'momentum': self.exe.arena_mom.cpu(), 'num_update': self.exe.num_update}
            if self.exe.loss_scale is not None:            # dynamic loss scaling: a resumed run goes on at this scale
                ls = self.exe.loss_scale['state'].cpu().tolist()
                states['loss_scale'], states['clean'] = float(ls[0]), int(ls[2])
            torch.save(states, '%s-%04d.states' % (prefix, epoch))

    # ---- optimizer (mx 'sgd' with multi_precision; lib/train_utils/utils.py:26-33)
    def init_optimizer(self, kvstore='local', optimizer='sgd', optimizer_params=(('learning_rate', 0.01),), force_init=False):
        if optimizer != 'sgd':
            raise NotImplementedError('optimizer %r (the reference trains with sgd)' % (optimizer,))
        op = dict(optimizer_params)
        guard = self._guard_options(op)
        guard['loss_scale'] = self._loss_scale_options(op.get('dynamic_loss_scale'))
        self.opt = {'lr': float(op.get('learning_rate', 0.01)), 'wd': float(op.get('wd', 0.0)),
                    'momentum': float(op.get('momentum', 0.0)), 'rescale_grad': float(op.get('rescale_grad', 1.0)),
                    'lr_scheduler': op.get('lr_scheduler')}
        self.opt.update(guard)
        self.opt['accumulate'] = self._accumulate_option(op)
        self.opt['skip_report'] = self._skip_report_option(op, guard['skip_nonfinite'] or guard['loss_scale'] is not None)
        if self.opt['lr_scheduler'] is not None:
            self.opt['lr_scheduler'].base_lr = self.opt['lr']
        self.optimizer_initialized = True
        self._guard_host = None
        self._loss_scale_resume = None
        self._accum_pending = self._accum_updates = 0
        for ex in getattr(self, '_exes', {}).values():
            self._guard_exe(ex)
            self._accum_exe(ex)

    # ---- gradient accumulation (Executor.set_accumulate): optimizer parameter accumulate = k, one update per k micro-batches on the
    # SUM of their gradients (k micro-batches = k ranks).  Without the key, SNIPER_ACCUMULATE is read here, once: the way the
    # reference's unchanged main_train.py turns it on.  The key wins over the variable.
    @staticmethod
    def _accumulate_option(op):
        from ..engine.executor import Executor
        if op.get('accumulate') is not None:              # (None is "absent", as for the guard's options)
            return Executor.check_accumulate(op['accumulate'])
        env = os.environ.get('SNIPER_ACCUMULATE')
        if env is None or not env.strip():
            return 1
        try:
            k = int(env.strip())
        except ValueError:
            raise ValueError('SNIPER_ACCUMULATE must be an int >= 1, got %r' % (env,))
        return Executor.check_accumulate(k)

    # ---- skip report (Executor.set_skip_report): optimizer parameter skip_report; without the key, SNIPER_SKIP_REPORT=1 turns it on
    # for the reference's unchanged main_train.py.  The key wins over the variable.
    @staticmethod
    def _skip_report_option(op, skips):
        v = op.get('skip_report')
        if v is None:
            env = (os.environ.get('SNIPER_SKIP_REPORT') or '').strip()
            if env not in ('', '0', '1'):
                raise ValueError('SNIPER_SKIP_REPORT must be 0 or 1, got %r' % (env,))
            v = env == '1'
        if not isinstance(v, (bool, np.bool_)) and v not in (0, 1):
            raise ValueError('optimizer parameter skip_report must be a bool, got %r' % (v,))
        if v and not skips:
            raise ValueError('skip_report needs skip_nonfinite (or dynamic_loss_scale): the report describes a skipped step')
        return bool(v)

    def _accum_exe(self, ex):
        """the optimizer's accumulate option -> a training executor (where _guard_exe is called); k = 1 on an executor that does not
        accumulate touches nothing"""
        opt = getattr(self, 'opt', None)
        if opt is None or not ex.for_training:
            return
        k = opt.get('accumulate', 1)
        if k > 1 or ex.accum is not None:
            ex.set_accumulate(k)

    def accumulate_state(self):
        """{'k': micro-batches per update, 'pending': micro-batches accumulated since the last update, 'updates': optimizer updates
        so far}.  Metrics, Speedometer and the guard's lagged snapshots stay per micro-batch / per update as they are."""
        opt = getattr(self, 'opt', None) or {}
        return {'k': int(opt.get('accumulate', 1)), 'pending': int(getattr(self, '_accum_pending', 0)),
                'updates': int(getattr(self, '_accum_updates', 0))}

    # ---- gradient guard (Executor.set_grad_guard): clip_gradient is mx 'sgd's parameter; clip_global_norm, skip_nonfinite and
    # max_consecutive_skips are this engine's
    @staticmethod
    def _guard_options(op):
        out = {}
        for key in ('clip_gradient', 'clip_global_norm'):
            v = op.get(key)
            if v is not None:
                if isinstance(v, bool) or not isinstance(v, (int, float, np.integer, np.floating)) or not float(v) > 0.0:
                    raise ValueError('optimizer parameter %s must be None or a number > 0, got %r' % (key, v))
                v = float(v)
            out[key] = v
        v = op.get('skip_nonfinite', False)
        if not isinstance(v, (bool, np.bool_)) and v not in (0, 1):
            raise ValueError('optimizer parameter skip_nonfinite must be a bool, got %r' % (v,))
        out['skip_nonfinite'] = bool(v)
        v = op.get('max_consecutive_skips', 16)
        if v is not None:
            if isinstance(v, bool) or not isinstance(v, (int, np.integer)) or int(v) < 1:
                raise ValueError('optimizer parameter max_consecutive_skips must be None or an int >= 1, got %r' % (v,))
            v = int(v)
        out['max_consecutive_skips'] = v
        out['guard'] = out['clip_gradient'] is not None or out['clip_global_norm'] is not None or out['skip_nonfinite']
        return out

    # ---- dynamic loss scaling (Executor.set_loss_scale): optimizer parameter dynamic_loss_scale = None / False, True, or a dict of
    # set_loss_scale's arguments.  Learning rate and weight decay are then the TRUE ones (nothing folded), clip_gradient and
    # clip_global_norm are in true units, and grad_guard_state()['norm'] is the true norm.
    _LOSS_SCALE_DEFAULTS = (('init_scale', 2.0 ** 16), ('growth_interval', 2000), ('growth_factor', 2.0), ('backoff_factor', 0.5),
                            ('min_scale', 1.0), ('max_scale', 2.0 ** 24), ('restore_aux', True))

    @classmethod
    def _loss_scale_options(cls, v):
        if v is None or v is False:
            return None
        if v is True:
            v = {}
        if not isinstance(v, dict):
            raise ValueError('optimizer parameter dynamic_loss_scale must be None, a bool or a dict, got %r' % (v,))
        out = dict(cls._LOSS_SCALE_DEFAULTS)
        unknown = sorted(set(v) - set(out))
        if unknown:
            raise ValueError('optimizer parameter dynamic_loss_scale: unknown keys %s (known: %s)' % (unknown, sorted(out)))
        out.update(v)

        from ..engine.executor import Executor
        Executor.check_loss_scale(**{k: out[k] for k in out if k != 'restore_aux'})
        for key in ('init_scale', 'growth_factor', 'backoff_factor', 'min_scale', 'max_scale'):
            out[key] = float(out[key])
        out['growth_interval'] = int(out['growth_interval'])
        if not isinstance(out['restore_aux'], (bool, np.bool_)):
            raise ValueError('dynamic_loss_scale: restore_aux must be a bool, got %r' % (out['restore_aux'],))
        out['restore_aux'] = bool(out['restore_aux'])
        return out

    def _guard_exe(self, ex):
        """the optimizer's guard and loss-scale options -> a training executor (at init_optimizer for the bound ones, at bind for later
        ones)"""
        opt = getattr(self, 'opt', None)
        if opt is None or not ex.for_training:
            return
        ls = opt.get('loss_scale')
        if ls is None and ex.loss_scale is not None:
            ex.set_loss_scale(None)                     # (first: while it is on, the guard cannot be turned off)
        if opt['guard'] or ex.guard is not None or ls is not None:
            ex.set_grad_guard(opt['clip_gradient'], opt['clip_global_norm'], opt['skip_nonfinite'] or ls is not None)
        if ls is not None:
            ex.set_loss_scale(**ls)
            resume = getattr(self, '_loss_scale_resume', None)
            if resume is not None:                      # load_optimizer_states: go on at the checkpoint's scale
                ex.loss_scale['state'][0] = float(resume[0])
                ex.loss_scale['state'][2] = float(resume[1])
        if opt.get('skip_report') or getattr(ex, 'skip_report', None) is not None:
            ex.set_skip_report(bool(opt.get('skip_report')))

    _LOSS_SCALE_KEYS = ('scale', 'scale_used', 'clean', 'growths', 'backoffs', 'held_max', 'held_min')

    @classmethod
    def _loss_scale_dict(cls, s):
        return dict(zip(cls._LOSS_SCALE_KEYS, (float(s[0]), float(s[1]), int(s[2]), int(s[3]), int(s[4]), int(s[5]), int(s[6]))))

    def loss_scale_state(self, wait=True):
        """The dynamic loss scaler's device state as a dict -- scale (what the next forward multiplies with), scale_used (what the
        gradients of the last step carried), clean steps since the scale changed, growths, backoffs, held_max, held_min -- or None
        when it is off.  wait as in grad_guard_state: True reads the device now, False returns the newest landed snapshot."""
        ls = self.exe.loss_scale if getattr(self, 'exe', None) is not None else None
        if ls is None:
            return None
        if wait:
            return self._loss_scale_dict(ls['state'].cpu().tolist())
        s = self._guard_landed()
        return self._loss_scale_dict(s[8:]) if s is not None and len(s) >= 16 else None

    def load_optimizer_states(self, fname):
        """A `.states` file of save_checkpoint(save_optimizer_states=True): the momentum arena and the update count; with dynamic
        loss scaling on, and a file that holds them, the loss scale and its clean-step count too (a file without them: the scale
        stays where it is)."""
        st = torch.load(fname, map_location='cpu')
        self.exe.arena_mom.copy_(st['momentum'].to(self.exe.arena_mom.device))
        self.exe.num_update = int(st['num_update'])
        if 'loss_scale' in st and self.opt.get('loss_scale') is not None:
            scale = float(st['loss_scale'])
            if not (scale > 0.0 and np.isfinite(scale) and np.frexp(scale)[0] == 0.5):
                raise ValueError('%s: loss_scale %r is not a positive power of two' % (fname, st['loss_scale']))
            self._loss_scale_resume = (scale, float(st.get('clean', 0)))
            for ex in self._exes.values():
                if ex.loss_scale is not None:
                    ex.loss_scale['state'][0] = scale
                    ex.loss_scale['state'][2] = self._loss_scale_resume[1]

    _GUARD_KEYS = ('norm', 'coef', 'skipped_last', 'nonfinite', 'steps', 'skipped', 'consecutive', 'sumsq')

    @classmethod
    def _guard_dict(cls, s):
        return dict(zip(cls._GUARD_KEYS, (float(s[0]), float(s[1]), bool(s[2]), int(s[3]), int(s[4]), int(s[5]), int(s[6]), float(s[7]))))

    def grad_guard_state(self, wait=True):
        """The guard's device state as a dict (norm and sumsq in the arena's units: with TRAIN.fp16 the gradients carry the static
        loss scale; with dynamic loss scaling on -- loss_scale_state -- norm is in TRUE units, divided by the scale the gradients
        carried, and only sumsq stays in the arena's), None when the guard is off.  wait=True reads the device now (waits for the steps enqueued so far);
        wait=False returns the newest snapshot that has already landed on the host -- one or two steps old -- or None before the first."""
        g = self.exe.guard if getattr(self, 'exe', None) is not None else None
        if g is None:
            return None
        if wait:
            return self._guard_dict(g['state'].cpu().tolist())
        s = self._guard_landed()
        return self._guard_dict(s) if s is not None else None

    def _guard_landed(self):
        """the newest snapshot that has landed on the host (looks only: update() does the inspecting), or None"""
        host = getattr(self, '_guard_host', None)
        if host is None:
            return None
        landed = [s['host'].tolist() for s in host['slots'] if s['event'] is not None and s['event'].query()]
        if host['last'] is not None:
            landed.append(host['last'])
        return max(landed, key=lambda s: s[4]) if landed else None

    def _guard_snapshot(self):
        """After a guarded step has been enqueued: its 64 bytes of state -> pinned host memory without waiting (a device copy on the
        step's stream -- the next step rewrites the state --, the device -> host copy on a side stream behind an event, as
        _snapshot_for_metric does for the outputs); then whatever EARLIER snapshot has landed is inspected: a skipped step is logged
        once, max_consecutive_skips skipped steps in a row raise FloatingPointError.  Never waits for the device."""
        g = self.exe.guard
        ls = self.exe.loss_scale
        nd_ = 16 if ls is not None else 8              # with dynamic loss scaling the scaler's eight doubles ride behind the guard's
        rep = getattr(self.exe, 'skip_report', None)
        nrep = rep['out'].numel() if rep is not None else 0
        host = getattr(self, '_guard_host', None)
        if host is not None and (host['slots'][0]['host'].numel() != nd_ or host['nrep'] != nrep):
            host = None
        if host is None:
            host = self._guard_host = {
                'stream': torch.cuda.Stream(device=self._device), 'k': 0, 'last': None, 'skipped': 0, 'steps': 0,
                'growths': 0, 'backoffs': 0, 'nrep': nrep, 'report': None,
                'slots': [{'dev': torch.zeros(nd_, dtype=torch.float64, device=g['state'].device),
                           'host': torch.zeros(nd_, dtype=torch.float64, pin_memory=True),
                           'event': None, 'fresh': False} for _ in range(2)]}
            if nrep:
                # the skip report rides with the state: cloned on the step's stream BETWEEN two optimizer passes, so a clone is the
                # report of one step, whole, and its header names that step
                for slot in host['slots']:
                    slot['rep_dev'] = torch.zeros_like(rep['out'])
                    slot['rep_host'] = torch.zeros(tuple(rep['out'].shape), dtype=torch.float64, pin_memory=True)
        self._guard_poll(host)                                 # (before the older slot is reused)
        slot = host['slots'][host['k'] & 1]
        host['k'] += 1
        main = torch.cuda.current_stream(self._device)
        if slot['event'] is not None:
            main.wait_event(slot['event'])                     # device-side: the slot's previous copy out has read slot['dev']
        if ls is not None:
            slot['dev'][:8].copy_(g['state'])
            slot['dev'][8:].copy_(ls['state'])
        else:
            slot['dev'].copy_(g['state'])
        if nrep:
            slot['rep_dev'].copy_(rep['out'])
        cloned = torch.cuda.Event()
        cloned.record(main)
        side = host['stream']
        side.wait_event(cloned)
        with torch.cuda.stream(side):
            slot['host'].copy_(slot['dev'], non_blocking=True)
            if nrep:
                slot['rep_host'].copy_(slot['rep_dev'], non_blocking=True)
            slot['event'] = torch.cuda.Event()
            slot['event'].record(side)
        slot['fresh'] = True

    def _guard_poll(self, host):
        for slot in sorted((s for s in host['slots'] if s['fresh'] and s['event'].query()), key=lambda s: float(s['host'][4])):
            slot['fresh'] = False
            s = slot['host'].tolist()
            if s[4] <= host['steps']:
                continue
            host['last'], host['steps'] = s, s[4]
            if s[5] > host['skipped']:
                host['skipped'] = s[5]
                if s[2]:
                    self.logger.warning('gradient guard: step %d skipped, %d non-finite gradient elements, norm of the finite rest %g '
                                        '(%d skipped of %d steps, %d in a row)', int(s[4]), int(s[3]), s[0], int(s[5]), int(s[4]), int(s[6]))
                    self._skip_report_log(host, slot, s)
                else:
                    self.logger.warning('gradient guard: %d of %d steps skipped so far', int(s[5]), int(s[4]))
            if len(s) >= 16:
                self._loss_scale_log(host, s)
            limit = self.opt.get('max_consecutive_skips')
            if limit is not None and s[6] >= limit:
                raise FloatingPointError('gradient guard: %d consecutive steps skipped for non-finite gradients (step %d, %d non-finite '
                                         'elements in the last one); max_consecutive_skips = %d' % (int(s[6]), int(s[4]), int(s[3]), limit))

    def _skip_report_log(self, host, slot, s):
        """the landed snapshot of a skipped step: its report (the header names this very step, or nothing is said) is kept for
        skip_report(wait=False) and up to three of its tensors are named in a second warning"""
        if 'rep_host' not in slot:
            return
        out = slot['rep_host'].numpy().copy()
        if out[0, 0] != 1.0 or out[0, 1] != s[4]:
            return
        host['report'] = out
        bad = self._report_dict(out, self.exe.skip_report['table']['names'])['tensors']
        text = ', '.join('%s (%d of %d, first at %d)' % (t['name'], t['nonfinite'], t['numel'], t['first_index']) for t in bad[:3])
        self.logger.warning('gradient guard: step %d skipped, non-finite gradients in %d tensors, first in %s%s', int(s[4]), len(bad), text,
                            ', ...' if len(bad) > 3 else '')

    @staticmethod
    def _report_dict(out, names):
        tensors = [{'name': name, 'nonfinite': int(r[2]), 'first_index': int(r[3]), 'max_abs': float(r[4]), 'norm': float(np.sqrt(r[0])),
                    'zeros': int(r[5]), 'numel': int(r[6])} for name, r in zip(names, out[1:]) if r[2] > 0]
        return {'step': int(out[0, 1]), 'tensors': tensors}

    def skip_report(self, wait=True):
        """Where the most recent skipped step had its non-finite gradients: {'step': the guard's step counter of that step,
        'tensors': [{'name', 'nonfinite', 'first_index', 'max_abs', 'norm', 'zeros', 'numel'}, ...]} -- the tensors with
        nonfinite > 0 only, in arena order; max_abs, norm and zeros describe the tensor's FINITE elements, in the arena's units (scaled
        with a loss scale).  first_index is an index into the arena's internal layout of the parameter (a convolution weight is stored
        [out][taps][in]), not into the reference-shaped array.  None when the report is off (optimizer parameter skip_report,
        TRAIN.SKIP_REPORT, SNIPER_SKIP_REPORT=1) or no step has been skipped yet.  wait=True reads the device now (waits for the steps
        enqueued so far); wait=False returns the newest report that has already landed on the host beside the guard's snapshots.
        Either way the report is one step's: it is written by that step's optimizer pass alone and read between passes."""
        ex = getattr(self, 'exe', None)
        rep = getattr(ex, 'skip_report', None)
        if rep is None:
            return None
        if wait:
            out = rep['out'].cpu().numpy()
        else:
            host = getattr(self, '_guard_host', None)
            out = host['report'] if host is not None else None
        if out is None or out[0, 0] != 1.0:
            return None
        return self._report_dict(out, rep['table']['names'])

    # ---- monitor (mx.mon.Monitor)
    def install_monitor(self, mon):
        """mon.install on the bound training executor; with a loss scale active the monitor's rows end with ('loss_scale', value):
        the scale the gradient rows carry."""
        assert self.binded, 'install_monitor: bind first'
        mon.install(self.exe)
        if self._monitor_scale_row not in mon.extra_rows:
            mon.extra_rows.append(self._monitor_scale_row)

    def _monitor_scale_row(self):
        ls = self.exe.loss_scale
        if ls is not None:
            # the optimizer pass moves the scale and leaves the one the gradients carried in [1]; inside an accumulation window no
            # pass has run since the forward, and [0] is still the scale in use
            st = ls['state'].cpu().tolist()
            ran = (getattr(self, 'opt', None) or {}).get('accumulate', 1) == 1 or getattr(self, '_accum_pending', 0) == 0
            return [('loss_scale', st[1] if ran and st[1] > 0 else st[0])]
        static = getattr(self, 'static_loss_scale', None)
        return [('loss_scale', float(static))] if static not in (None, 1.0) else []

    @staticmethod
    def _monitor_from_env():
        env = os.environ.get('SNIPER_MONITOR')
        if env is None or not env.strip():
            return None
        from .mon import Monitor, parse_monitor_env
        interval, pattern = parse_monitor_env(env)
        return Monitor(interval, pattern=pattern)

    def _loss_scale_log(self, host, s):
        """one landed snapshot (guard's eight doubles, then the scaler's): a back-off is a warning, a growth an info line, once each"""
        scale, used, growths, backoffs = s[8], s[9], s[11], s[12]
        if backoffs > host['backoffs']:
            if s[2] and backoffs == host['backoffs'] + 1:
                self.logger.warning('loss scale: step %d skipped, %d non-finite gradient elements: scale %g -> %g (%d back-offs)',
                                    int(s[4]), int(s[3]), used, scale, int(backoffs))
            else:
                self.logger.warning('loss scale: %d back-offs so far (step %d), scale now %g', int(backoffs), int(s[4]), scale)
            host['backoffs'] = backoffs
        if growths > host['growths']:
            self.logger.info('loss scale: step %d, scale %g -> %g (%d growths)', int(s[4]), used, scale, int(growths))
            host['growths'] = growths

    # ---- compute
    def _adopt_iterator(self, train_data):
        """An iterator whose class sniper_amd.ext.rank_slice wrapped assembles only this rank's slice of every global batch:
        its batches (and provide_data) are rank-local -- nothing to slice, nothing to divide -- but the ranks must still walk
        the SAME chip database (_sync_epoch)."""
        from ..ext import rank_slice
        if self.world > 1 and rank_slice.is_rank_sliced(train_data):
            self.slice_inputs = False
            self._global_iter = True

    def _slice(self, a):
        if self.world > 1 and self.slice_inputs:
            n = a.shape[0] // self.world
            return a[self.rank * n:(self.rank + 1) * n]
        return a

    def _feed(self, data_batch):
        if getattr(data_batch, 'ready_event', None) is not None:       # assembled on the prefetch worker's stream
            from ..iterators.PrefetchingIter import adopt_batch
            adopt_batch(data_batch)
        feed = {}
        for name, arr in zip(self.data_names, data_batch.data):
            feed[name] = self._slice(arr)
        if data_batch.label is not None:
            for name, arr in zip(self.label_names, data_batch.label):
                feed[name] = self._slice(arr)
        self._labels = [self._slice(a) for a in (data_batch.label or [])]
        return {k: v for k, v in feed.items() if k in self.exe.input_names}

    def forward(self, data_batch, is_train=None):
        feed = self._feed(data_batch)
        if not self.for_training:
            feed = {k: self._bucket(v, self.__dict__.setdefault('_bucket_bufs', {}), k) for k, v in feed.items()}
            shapes = {k: tuple(v.shape) for k, v in feed.items()}
            if any(tuple(self.exe.vals_shape(k)) != s for k, s in shapes.items()):
                self.exe = self._exe_for(shapes)                       # rebind for this batch shape (MXNet reshapes too)
        self.exe.forward(feed, is_train=self.for_training if is_train is None else is_train)

    @staticmethod
    def _bucket(a, cache=None, key=None, q=64):
        """Test-time image batches are zero padded to the batch maximum anyway (MNIteratorTestAutoFocus._get_batch);
        padding H, W further up to a multiple of 64 keeps the number of distinct bound shapes small.  im_info carries
        the true sizes, so decoding and clipping are unaffected.
        cache (this Module's, per input name): the padded buffer of a bucket shape is allocated and zeroed ONCE; a batch is copied
        into its corner and only the strips a previous, larger batch left behind are cleared -- a fresh torch.zeros per batch was
        3 ms of host time (and a fill kernel over the whole buffer) per 8-image pass.  Safe per Module: every use is enqueued on the
        Module's stream before the executor copies the buffer into its bound input."""
        t = a._data if hasattr(a, '_data') else a
        if not (isinstance(t, torch.Tensor) and t.dim() == 4):
            return a
        H, W = int(t.shape[2]), int(t.shape[3])
        Hb, Wb = -(-H // q) * q, -(-W // q) * q
        if (Hb, Wb) == (H, W):
            return a
        shape = (int(t.shape[0]), int(t.shape[1]), Hb, Wb)
        if cache is None:
            out = torch.zeros(shape, dtype=t.dtype, device=t.device)
        else:
            ent = cache.get((key, shape, t.dtype, t.device))
            if ent is None:
                ent = cache[(key, shape, t.dtype, t.device)] = [torch.zeros(shape, dtype=t.dtype, device=t.device), 0, 0]
            out, h0, w0 = ent
            if h0 > H:
                out[:, :, H:h0, :].zero_()
            if w0 > W:
                out[:, :, :H, W:w0].zero_()
            ent[1], ent[2] = H, W
        out[:, :, :H, :W] = t
        return nd.NDArray(out)

    def backward(self, out_grads=None):
        self.exe.backward()

    def forward_backward(self, data_batch):
        """The training step's compute: one hipGraph replay once the executor has captured it (two with a split
        backward: the first segment's gradient all-reduce is started between them)."""
        self._comm_event = None
        # accumulating: no overlap -- the first segment's all-reduce would run per micro-step and be summed k times for nothing
        overlap = self.exe.split_k and (getattr(self, 'opt', None) or {}).get('accumulate', 1) == 1
        self.exe.forward_backward(self._feed(data_batch), between=self._allreduce_first_segment if overlap else None)

    def _half_buf(self):
        exe = self.exe
        if getattr(exe, '_half_buf', None) is None:
            n = max([b for _, half, _, b in exe.ar_ranges if half] or [0])
            exe._half_buf = torch.empty(max(n, 8), dtype=torch.float16, device=exe.arena_grad.device)
        return exe._half_buf

    def _allreduce_first_segment(self):
        """Gradients of the steps behind the split (heads, RPN, late trunk) are final: sum them over the ranks on a
        communication stream while the main stream runs the second backward segment (disjoint arena ranges)."""
        from ..parallel import allreduce_ranges
        d = _dist()
        if d is None or d.get_world_size() == 1:
            return
        exe = self.exe
        if getattr(self, '_comm_stream', None) is None:
            self._comm_stream = torch.cuda.Stream(device=exe.arena_grad.device)
        probe = getattr(self, '_comm_probe', None)       # bench.py: a list -> timed events of this step's overlap (else untimed events)
        ready = torch.cuda.Event(enable_timing=probe is not None)
        ready.record(torch.cuda.current_stream())
        self._comm_stream.wait_event(ready)
        with torch.cuda.stream(self._comm_stream):
            allreduce_ranges(exe.grad_arena(), [(h, a, b) for ph, h, a, b in exe.ar_ranges if ph == 0], d, self._half_buf())
            self._comm_event = torch.cuda.Event(enable_timing=probe is not None)
            self._comm_event.record(self._comm_stream)
        if probe is not None:
            probe.append({'seg2_start': ready, 'comm_end': self._comm_event})

    def update(self):
        from ..parallel import allreduce_ranges
        k = self.opt.get('accumulate', 1)
        if k > 1:
            # one micro-step of a window of k: its gradients go into the accumulation arena; until the k-th nothing else happens (no
            # all-reduce, no scheduler call, no optimizer launch, no snapshot).  The k-th all-reduces the SUM once (grad_arena() is
            # the accumulation arena) and updates.  The window ignores epochs: a partial one carries over.
            self._accum_pending = self.exe.accumulate()
            if self._accum_pending < k:
                return
        d = _dist()
        if d is not None and d.get_world_size() > 1:          # sum over ranks == kvstore 'device' push/pull
            exe = self.exe
            first_done = getattr(self, '_comm_event', None) is not None
            probe = getattr(self, '_comm_probe', None)
            if probe and first_done and 'seg2_end' not in probe[-1]:
                e = torch.cuda.Event(enable_timing=True)       # the second backward segment has been enqueued: its end on the main stream
                e.record(torch.cuda.current_stream())
                probe[-1]['seg2_end'] = e
            rest = [(h, a, b) for ph, h, a, b in exe.ar_ranges if not (first_done and ph == 0)]
            allreduce_ranges(exe.grad_arena(), rest, d, self._half_buf())
            if first_done:
                torch.cuda.current_stream().wait_event(self._comm_event)
                self._comm_event = None
        sched = self.opt['lr_scheduler']
        lr = sched(self.exe.num_update + 1) if sched is not None else self.opt['lr']
        # (the guard, when set, is the first thing the optimizer pass runs: behind the all-reduce, so every rank decides on the same sum)
        self.exe.update(lr, self.opt['wd'], self.opt['momentum'], self.opt['rescale_grad'])
        self._accum_pending = 0
        self._accum_updates = getattr(self, '_accum_updates', 0) + 1
        if self.exe.guard is not None:
            self._guard_snapshot()

    def get_outputs(self, merge_multi_context=True):
        """The executor's output tensors, NOT copies: a test-time executor replays a captured forward into the same tensors, so
        what this returned for batch i is overwritten by forward(i + 1) -- asnumpy() / copy what must outlive the next forward
        (Tester copies to pinned host memory on the same stream before it launches the next batch)."""
        outs = [nd.NDArray(t) for t in self.exe.outputs]
        if merge_multi_context:
            return outs
        return [[o] for o in outs]

    def update_metric(self, eval_metric, labels):
        eval_metric.update(labels, self.get_outputs())

    def _snapshot_for_metric(self, slot):
        """Outputs and labels of the step just enqueued -> pinned host copies (two alternating sets), without waiting: a device
        clone on the step's stream (the next replay overwrites the outputs), the device -> host copy on a side stream."""
        st = self.__dict__.setdefault('_metric_state', {'stream': torch.cuda.Stream(device=self._device), 'sets': {}})
        tensors = [('o', i, t) for i, t in enumerate(self.exe.outputs)]
        host_labels = {}
        for i, a in enumerate(self._labels):
            d = a._data if isinstance(a, nd.NDArray) else a
            if isinstance(d, torch.Tensor) and d.is_cuda:
                tensors.append(('l', i, d))
            else:
                host_labels[i] = a if isinstance(a, nd.NDArray) else nd.NDArray(np.asarray(d))
        bufs = st['sets'].setdefault(slot, {})
        main = torch.cuda.current_stream(self._device)
        staged = []
        for kind, i, t in tensors:
            key = (kind, i, tuple(t.shape), t.dtype)
            ent = bufs.get(key)
            if ent is None:
                ent = bufs[key] = (torch.empty_like(t), torch.empty(tuple(t.shape), dtype=t.dtype, pin_memory=True))
            ent[0].copy_(t)                                   # on the step's stream: ordered before the next replay
            staged.append((kind, i, ent))
        cloned = torch.cuda.Event()
        cloned.record(main)
        side = st['stream']
        side.wait_event(cloned)
        with torch.cuda.stream(side):
            for _, _, (dcopy, hcopy) in staged:
                hcopy.copy_(dcopy, non_blocking=True)
            done = torch.cuda.Event()
            done.record(side)
        return staged, host_labels, done

    def _update_metric_from(self, eval_metric, snap):
        staged, host_labels, done = snap
        done.synchronize()
        outs, labels = {}, dict(host_labels)
        for kind, i, (_, hcopy) in staged:
            a = hcopy.float().numpy() if hcopy.dtype in (torch.float16, torch.bfloat16) else hcopy.numpy()
            (outs if kind == 'o' else labels)[i] = nd.NDArray(a)
        eval_metric.update([labels[i] for i in sorted(labels)], [outs[i] for i in sorted(outs)])

    def _sync_epoch(self, train_data, epoch):
        """Data parallel with a GLOBAL-batch iterator (slice_inputs): every rank builds the epoch's chip database itself, from
        numpy's global RNG (chip stride, chip permutations, negative-chip choice, index shuffle -- MNIteratorE2E.reset).  All
        ranks must build the SAME one, or rank r's slice r belongs to a different batch and the per-step all-reduces pair
        different steps: rank 0's seed is broadcast, numpy is re-seeded, the iterator reset, and the epoch length checked."""
        d = _dist()
        if d is None or d.get_world_size() == 1 or not (self.slice_inputs or getattr(self, '_global_iter', False)):
            return False
        dev = getattr(self, '_device', None) or torch.device('cpu')
        t = torch.zeros(1, dtype=torch.int64, device=dev)
        if self.rank == 0:
            t[0] = int(np.random.randint(0, 2 ** 31 - 1))
        d.broadcast(t, src=0)
        np.random.seed((int(t.item()) + epoch) % (2 ** 31 - 1))
        train_data.reset()
        n = torch.tensor([len(train_data), -len(train_data)], dtype=torch.int64, device=dev) if hasattr(train_data, '__len__') \
            else None
        if n is not None:
            d.all_reduce(n, op=d.ReduceOp.MAX)
            if int(n[0]) != -int(n[1]):
                raise RuntimeError('data-parallel ranks built epochs of different length (%d..%d batches worth of chips): the '
                                   'iterators are not synchronised' % (-int(n[1]), int(n[0])))
        return True

    # ---- training loop (main_train.py:143-146)
    def fit(self, train_data, eval_data=None, eval_metric='acc', epoch_end_callback=None, batch_end_callback=None,
            kvstore='local', optimizer='sgd', optimizer_params=(('learning_rate', 0.01),), eval_end_callback=None,
            eval_batch_end_callback=None, initializer=None, arg_params=None, aux_params=None, allow_missing=False,
            force_rebind=False, force_init=False, begin_epoch=0, num_epoch=None, validation_metric=None, monitor=None):
        assert num_epoch is not None, 'please specify number of epochs'
        self._adopt_iterator(train_data)
        self.bind(data_shapes=train_data.provide_data, label_shapes=train_data.provide_label, for_training=True,
                  force_rebind=force_rebind)
        self.init_params(initializer=initializer, arg_params=arg_params, aux_params=aux_params, allow_missing=allow_missing,
                         force_init=force_init)
        self.init_optimizer(kvstore=kvstore, optimizer=optimizer, optimizer_params=optimizer_params)
        # mx.mon.Monitor: tic() before forward_backward; update(), the metric and the batch-end callbacks; then toc_print().  Without the
        # argument SNIPER_MONITOR=<interval>[:<regex>] makes one (the reference's main_train.py passes none).
        if monitor is None:
            monitor = self._monitor_from_env()
        if monitor is not None:
            self.install_monitor(monitor)
        cbs = lambda c: c if isinstance(c, (list, tuple)) else ([c] if c is not None else [])
        for epoch in range(begin_epoch, num_epoch):
            tic = time.time()
            if hasattr(eval_metric, 'reset'):
                eval_metric.reset()
            nbatch = 0
            if self._sync_epoch(train_data, epoch):
                pass                              # the iterator was re-seeded and reset on every rank
            elif epoch > begin_epoch:
                train_data.reset()
            # The reference's metrics read every output with asnumpy() (lib/train_utils/metric.py:50-369).  Under MXNet that waits
            # for the FORWARD outputs only and the backward pass runs on beneath the host's numpy; here a step is one captured
            # graph on one stream, so reading batch k's outputs right away would wait for the whole step and leave the GPU idle
            # while the host computes metrics and enqueues batch k + 1 (measured: 27.5 ms per batch for a 22.9 ms step,
            # profiles/r05_fit_path.txt).  So: outputs + labels of batch k are snapshotted on the device, copied to pinned host
            # memory on a side stream, and the metrics of batch k are updated one iteration later -- when the copy has long
            # landed and batch k + 1 is already queued.  The running metrics a batch_end_callback sees therefore cover the
            # batches up to k - 1 (the epoch-end values cover all); SNIPER_METRIC_LAG=0: update at once, as before.
            lag = os.environ.get('SNIPER_METRIC_LAG', '1') != '0' and getattr(self, '_device', None) is not None and \
                self._device.type == 'cuda' and hasattr(eval_metric, 'update')
            held = None
            for data_batch in train_data:
                if monitor is not None:
                    monitor.tic()
                self.forward_backward(data_batch)
                self.update()
                if lag:
                    snap = self._snapshot_for_metric(nbatch & 1)
                    if held is not None:
                        self._update_metric_from(eval_metric, held)
                    held = snap
                elif hasattr(eval_metric, 'update'):
                    self.update_metric(eval_metric, self._labels)
                if batch_end_callback is not None:
                    param = BatchEndParam(epoch=epoch, nbatch=nbatch, eval_metric=eval_metric, locals=locals())     # (once per batch)
                    for cb in cbs(batch_end_callback):
                        cb(param)
                if monitor is not None:
                    monitor.toc_print()
                nbatch += 1
            if held is not None:
                self._update_metric_from(eval_metric, held)
                held = None
            if hasattr(eval_metric, 'get_name_value'):
                for name, val in eval_metric.get_name_value():
                    self.logger.info('Epoch[%d] Train-%s=%f', epoch, name, val)
            self.logger.info('Epoch[%d] Time cost=%.3f', epoch, time.time() - tic)
            arg, aux = self.get_params()
            if self.rank == 0:                    # replicas are identical: one writer (do_checkpoint / the symbols' checkpoint_callback)
                for cb in cbs(epoch_end_callback):
                    cb(epoch, self.symbol, arg, aux)
            d = _dist()
            if d is not None and d.get_world_size() > 1:
                d.barrier()
