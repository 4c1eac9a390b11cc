"""The COTR model object, MI355X edition.

Same seam as the reference (``COTR/models/cotr_model.py:15-51``): ``build(args)`` returns an
``nn.Module`` whose ``state_dict()`` has the reference's keys (a reference checkpoint loads
with ``utils.safe_load_weights``), which exposes ``.transformer .corr_embed .query_proj
.input_proj .backbone`` (``train_cotr.py:49-55``) and whose
``forward(samples, queries) -> {'pred_corrs': [B,Q,2]}`` is what ``SparseEngine.infer_batch``
(``COTR/inference/sparse_engine.py:47-56``) and friends call.

The sub-modules here are PARAMETER CONTAINERS only.  All arithmetic of ``forward`` runs in
``libcotr_hip.so`` (hand-written gfx950 kernels, ``cotr_amd/csrc``) through the C ABI of
``include/cotr_hip.h``; there is no PyTorch or CPU fallback - calling the model with CPU
tensors, or without the built library, raises.
"""
import ctypes

import numpy as np
import torch
from torch import nn

from .. import _lib
from .misc import NestedTensor
from .spec import LAYER_CHANNELS, resnet_stages

MAX_SIZE = 256  # COTR/utils/constants.py:2


class FrozenBatchNorm2d(nn.Module):
    """Four fixed buffers per norm (COTR/models/backbone.py:21-44); applied inside the HIP
    convolution epilogue as x*scale+bias with scale = w*rsqrt(var+1e-5) (backbone.py:46-56)."""

    def __init__(self, n):
        super().__init__()
        self.register_buffer('weight', torch.ones(n))
        self.register_buffer('bias', torch.zeros(n))
        self.register_buffer('running_mean', torch.zeros(n))
        self.register_buffer('running_var', torch.ones(n))

    def _load_from_state_dict(self, state_dict, prefix, *rest):
        state_dict.pop(prefix + 'num_batches_tracked', None)  # torchvision checkpoints carry it
        super()._load_from_state_dict(state_dict, prefix, *rest)


def _conv(cin, cout, k, stride):
    return nn.Conv2d(cin, cout, k, stride=stride, padding=k // 2, bias=False)


class _Bottleneck(nn.Module):
    def __init__(self, inplanes, planes, stride, downsample):
        super().__init__()
        self.conv1, self.bn1 = _conv(inplanes, planes, 1, 1), FrozenBatchNorm2d(planes)
        self.conv2, self.bn2 = _conv(planes, planes, 3, stride), FrozenBatchNorm2d(planes)
        self.conv3, self.bn3 = _conv(planes, planes * 4, 1, 1), FrozenBatchNorm2d(planes * 4)
        if downsample:
            self.downsample = nn.Sequential(_conv(inplanes, planes * 4, 1, stride), FrozenBatchNorm2d(planes * 4))


class _ResNetBody(nn.Module):
    """Parameters of torchvision resnet50 children conv1 .. ``layer`` (what the reference's
    IntermediateLayerGetter keeps, COTR/models/backbone.py:71)."""

    def __init__(self, layer):
        super().__init__()
        self.conv1, self.bn1 = _conv(3, 64, 7, 2), FrozenBatchNorm2d(64)
        inplanes = 64
        for name, planes, blocks, stride in resnet_stages(layer):
            seq = nn.Sequential(*[_Bottleneck(inplanes if b == 0 else planes * 4, planes,
                                              stride if b == 0 else 1, b == 0) for b in range(blocks)])
            setattr(self, name, seq)
            inplanes = planes * 4
        for m in self.modules():
            if isinstance(m, nn.Conv2d):
                nn.init.kaiming_normal_(m.weight, mode='fan_out', nonlinearity='relu')


class _Backbone(nn.Module):
    def __init__(self, layer, train_backbone):
        super().__init__()
        self.body = _ResNetBody(layer)
        self.num_channels = LAYER_CHANNELS[layer]
        for name, p in self.body.named_parameters():  # COTR/models/backbone.py:66-69
            if not train_backbone or ('layer2' not in name and 'layer3' not in name and 'layer4' not in name):
                p.requires_grad_(False)


class _NoParams(nn.Module):
    """Stand-in for the parameter-free encodings (``query_proj``, ``backbone[1]``)."""

    def __init__(self, what):
        super().__init__()
        self.what = what

    def extra_repr(self):
        return self.what


class _EncoderLayer(nn.Module):
    def __init__(self, d, heads, ffn, dropout):
        super().__init__()
        self.self_attn = nn.MultiheadAttention(d, heads, dropout=dropout)
        self.linear1, self.linear2 = nn.Linear(d, ffn), nn.Linear(ffn, d)
        self.norm1, self.norm2 = nn.LayerNorm(d), nn.LayerNorm(d)


class _DecoderLayer(nn.Module):
    def __init__(self, d, heads, ffn, dropout):
        super().__init__()
        self.multihead_attn = nn.MultiheadAttention(d, heads, dropout=dropout)
        self.linear1, self.linear2 = nn.Linear(d, ffn), nn.Linear(ffn, d)
        # norm1 is a parameter of the reference that its forward never applies (transformer.py:173)
        self.norm1, self.norm2, self.norm3 = nn.LayerNorm(d), nn.LayerNorm(d), nn.LayerNorm(d)


class _Stack(nn.Module):
    def __init__(self, layers, norm=None):
        super().__init__()
        self.layers = nn.ModuleList(layers)
        if norm is not None:
            self.norm = norm


class _Transformer(nn.Module):
    def __init__(self, d, heads, enc_layers, dec_layers, ffn, dropout):
        super().__init__()
        self.encoder = _Stack([_EncoderLayer(d, heads, ffn, dropout) for _ in range(enc_layers)])
        self.decoder = _Stack([_DecoderLayer(d, heads, ffn, dropout) for _ in range(dec_layers)], nn.LayerNorm(d))
        self.d_model, self.nhead = d, heads
        for p in self.parameters():  # COTR/models/transformer.py:42-45
            if p.dim() > 1:
                nn.init.xavier_uniform_(p)


class _MLP(nn.Module):
    def __init__(self, dims):
        super().__init__()
        self.num_layers = len(dims) - 1
        self.layers = nn.ModuleList(nn.Linear(a, b) for a, b in zip(dims[:-1], dims[1:]))


class _Workspace:
    """The scratch a model hands to its library handle (cotr_set_workspace) and what it was sized for.  The library's encode cache +
    scratch come from torch's caching allocator: a larger batch then costs one torch allocation instead of hipFree + hipMalloc
    (device synchronisations) inside the library.  Per process like the handle: never pickled / deep-copied (COTR.__getstate__)."""

    def __init__(self):
        self.buffer = None      # uint8 tensor; the library gets its first 256-byte boundary
        self.shape = (0, 0)     # (pairs, queries) it serves
        self.varlen = False     # sized for varlen calls of that many pairs and pairs * queries rows as well; remembered once asked for
        self.images = 0         # sized for pairs calls of up to that many distinct images as well; the largest count asked for
        self.stale = False      # a knob changed: the library's carving of the buffer is re-done at the next call
        self.pins = set()       # ids of captured graphs that have the buffer's addresses baked in (COTR.pin_workspace)

    def ensure(self, lib, handle, device, b, q, keep_encode=False, varlen=False, images=0):
        """Serve a call of b pairs x q queries; False when that dropped the library's cached encode.  The workspace only grows; with
        keep_encode a cached encode is carried over into a new one (stream-ordered device copy; the old tensor goes back to torch's
        pool, which is stream-ordered too)."""
        b, q = max(b, self.shape[0]), max(q, self.shape[1])
        m = max(images, self.images)
        if self.buffer is not None and (b, q) == self.shape and not self.stale and (self.varlen or not varlen) and m == self.images:
            return True
        need = ctypes.c_size_t()
        if varlen or self.varlen:       # the decoder scratch plus the tile tables
            offsets = (ctypes.c_int * (b + 1))(*[i * max(q, 1) for i in range(b + 1)])
            _lib.check(lib.cotr_scratch_bytes_varlen(handle, offsets, b, ctypes.byref(need)), handle, 'cotr_scratch_bytes_varlen')
            self.varlen = True
        else:
            _lib.check(lib.cotr_scratch_bytes(handle, b, max(q, 1), ctypes.byref(need)), handle, 'cotr_scratch_bytes')
        if m:
            need_p = ctypes.c_size_t()
            _lib.check(lib.cotr_scratch_bytes_pairs(handle, m, b, max(q, 1), ctypes.byref(need_p)), handle, 'cotr_scratch_bytes_pairs')
            need.value = max(need.value, need_p.value)
            self.images = m
        kept = True
        if self.buffer is None or self.buffer.numel() < need.value + 256:
            if self.buffer is not None and self.pins:
                raise _lib.CotrHipError(
                    f'the workspace would have to grow to {need.value} bytes for {b} pairs x {q} queries, but a captured training '
                    'step (GraphedTrainStep) has its addresses baked in: call model.reserve(max_pairs, max_queries) BEFORE '
                    'capturing, or close() the captured step first')
            ws = torch.empty(need.value + 256, dtype=torch.uint8, device=device)
            self.release(device)
            kept = bool(keep_encode and self.buffer is not None and b == self.shape[0])     # same pairs, more queries: the cached encode moves along
            self._hand_over(lib, handle, ws, need.value, int(kept))
            self.buffer = ws
        elif self.stale and not self.pins:
            # same buffer, new knobs: the three regions grow in place and never shrink, so regions carved under the old knobs plus one
            # that is larger under the new ones can exceed what cotr_scratch_bytes promises for either - start the carving afresh
            self._hand_over(lib, handle, self.buffer, self.buffer.numel() - 256, 0)
            kept = False
        self.stale = False
        self.shape = (b, q)
        return kept

    @staticmethod
    def _hand_over(lib, handle, ws, nbytes, keep):
        off = (-ws.data_ptr()) % 256
        _lib.check(lib.cotr_set_workspace(handle, ctypes.c_void_p(ws.data_ptr() + off), nbytes, keep, _lib.current_stream_ptr()),
                   handle, 'cotr_set_workspace')

    def release(self, device=None):
        """The buffer is about to go back to torch's caching allocator, which may hand it out on ANOTHER stream while kernels
        enqueued here still use it."""
        if self.buffer is not None:
            self.buffer.record_stream(torch.cuda.current_stream(device or self.buffer.device))


class COTR(nn.Module):
    def __init__(self, args):
        super().__init__()
        d = args.hidden_dim
        layer = getattr(args, 'layer', 'layer3')
        ffn = args.dim_feedforward
        unsupported = []
        if args.backbone != 'resnet50': unsupported.append(f'backbone={args.backbone}')
        if layer != 'layer3' or ffn != 1024: unsupported.append(f'layer={layer}/dim_feedforward={ffn}')
        if d != 256 or args.nheads != 8: unsupported.append(f'hidden_dim={d}/nheads={args.nheads}')
        if args.dilation: unsupported.append('dilation')
        if args.position_embedding != 'lin_sine': unsupported.append(f'position_embedding={args.position_embedding}')
        if unsupported:
            raise NotImplementedError(
                'libcotr_hip implements COTR\'s published configuration (resnet50/layer3, hidden 256, 8 heads, '
                'lin_sine; COTR/options/options.py:41-51); not: ' + ', '.join(unsupported))
        self.transformer = _Transformer(d, args.nheads, args.enc_layers, args.dec_layers, ffn, args.dropout)
        self.corr_embed = _MLP([d, d, d, 2])
        self.query_proj = _NoParams('lin_sine, depth 64')
        self.input_proj = nn.Conv2d(LAYER_CHANNELS[layer], d, kernel_size=1)
        train_backbone = getattr(args, 'lr_backbone', 0) > 0
        self.backbone = nn.Sequential(_Backbone(layer, train_backbone), _NoParams('lin_sine image grid encoding'))
        self.backbone.num_channels = LAYER_CHANNELS[layer]
        self._handle = None
        self._handle_device = None
        self._weights_dirty = True
        self._encoded_batch = 0
        self._workspace = _Workspace()     # scratch handed to the library (torch caching allocator)
        self._knobs = {}            # tuning knobs of THIS model's handle (set_knob); re-applied when the handle is re-created

    # ------------------------------------------------------------------ weight synchronisation
    def _apply(self, fn, *a, **kw):  # .cuda() / .to() / .float() move or replace the storage
        self._weights_dirty = True
        return super()._apply(fn, *a, **kw)

    def load_state_dict(self, *a, **kw):
        self._weights_dirty = True
        return super().load_state_dict(*a, **kw)

    def refresh_weights(self):
        """Re-pack the weights into the HIP library at the next call (needed only after
        modifying parameters in place; .to()/.cuda()/load_state_dict() do it themselves)."""
        self._weights_dirty = True

    def _ensure_ready(self, device):
        lib = _lib.load_library()
        if device.type != 'cuda':
            raise _lib.CotrHipError(
                'cotr_amd runs the COTR forward path on an MI355X only (HIP kernels, no CPU/PyTorch '
                f'fallback); got tensors on {device}. Move the model and inputs with .cuda().')
        index = device.index if device.index is not None else torch.cuda.current_device()
        if self._handle is None or self._handle_device != index:
            self._release()
            handle = ctypes.c_void_p()
            _lib.check(lib.cotr_create(ctypes.byref(handle), index), None, 'cotr_create')
            try:                                          # the remembered knobs go on BEFORE the handle is published: a knob the library
                for name, value in self._knobs.items():   # refuses must not leave a half-configured handle behind
                    _lib.set_knob(name, value, handle)
            except Exception:
                lib.cotr_destroy(handle)
                raise
            self._handle, self._handle_device = handle, index
            self._weights_dirty = True
            # the new handle gets a new buffer; varlen / images / stale stay, so that it is sized at once for the kinds of call this model makes
            self._workspace.buffer, self._workspace.shape = None, (0, 0)
        if self._weights_dirty:
            sd = {k: v.detach() for k, v in self.state_dict().items()}
            bad = [k for k, v in sd.items() if v.dtype != torch.float32]
            if bad:
                raise _lib.CotrHipError(f'libcotr_hip is fp32 (1e-3 px parity bar); non-fp32 tensors: {bad[:3]}...')
            keep = [v.contiguous() for v in sd.values()]
            n = len(keep)
            names = (ctypes.c_char_p * n)(*[k.encode() for k in sd])
            ptrs = (ctypes.c_void_p * n)(*[t.data_ptr() for t in keep])
            numels = (ctypes.c_int64 * n)(*[t.numel() for t in keep])
            torch.cuda.synchronize(index)
            _lib.check(lib.cotr_load_weights(self._handle, names, ptrs, numels, n), self._handle, 'cotr_load_weights')
            self._weights_dirty = False
            self._encoded_batch = 0
        return lib

    def _call(self, name, device, shape, args, encoded=None, keep_encode=False, varlen=False, images=0):
        """Every library call of the model: the handle and its weights, the workspace for shape = (pairs, queries), then
        lib.<name>(handle, *args, stream) on the caller's current stream.  keep_encode: the call reads the cached encode of `pairs`
        pairs.  encoded: the pairs the call leaves in the encode cache (None: it leaves the record as it is)."""
        lib = self._ensure_ready(device)
        with torch.cuda.device(device):
            self._size_workspace(lib, device, *shape, keep_encode=keep_encode, varlen=varlen, images=images)
            if keep_encode and self._encoded_batch != shape[0]:
                raise _lib.CotrHipError(f'{name[5:]} of {shape[0]} pairs: the cached encode was dropped by a workspace change')
            _lib.check(getattr(lib, name)(self._handle, *args, _lib.current_stream_ptr()), self._handle, name)
        if encoded is not None:
            self._encoded_batch = encoded

    def _size_workspace(self, lib, device, b, q, **flags):
        if not self._workspace.ensure(lib, self._handle, device, b, q, **flags):
            self._encoded_batch = 0         # the library dropped its cached encode with the old carving

    def _release(self):
        handle = self.__dict__.get('_handle')
        if handle is not None:
            self.__dict__['_handle'] = None  # (nn.Module.__setattr__ may already be torn down at interpreter exit)
            try:
                _lib.load_library().cotr_destroy(handle)
            except Exception:
                pass

    def __del__(self):
        self._release()

    def __getstate__(self):  # the HIP handle is per process: never pickled / deep-copied
        state = self.__dict__.copy()
        state['_handle'], state['_handle_device'], state['_weights_dirty'], state['_encoded_batch'] = None, None, True, 0
        state['_workspace'], state['_knobs'] = _Workspace(), dict(self._knobs)
        return state

    def __setstate__(self, state):
        super().__setstate__(state)
        if not isinstance(state.get('_workspace'), _Workspace):    # a pickle from before the workspace object
            self._workspace = _Workspace()
        self.__dict__.setdefault('_knobs', {})

    # ------------------------------------------------------------------ the path
    def _check_mode(self):
        if self.training:
            raise NotImplementedError('encode()/decode() are the inference split (model.eval()); in training mode call '
                                      'model(img, queries) - see cotr_amd/training.py')

    def train(self, mode=True):
        # parameters updated by an optimiser while training must be re-packed into the HIP library before the next
        # inference call (the frozen backbone the training step uses is not touched by the optimiser)
        if self.training and not mode:
            self._weights_dirty = True
        return super().train(mode)

    @staticmethod
    def _as_batch(samples):
        if isinstance(samples, NestedTensor):
            # the reference turns a NestedTensor mask into a key-padding mask (transformer.py:49-55); every caller of
            # the reference feeds exactly 256x512 pixels, i.e. an all-False mask, and the HIP path has no masked
            # attention - refuse a real mask instead of silently ignoring it
            if samples.mask is not None and bool(samples.mask.any()):
                raise NotImplementedError('libcotr_hip has no key-padding mask: NestedTensor.mask must be all False '
                                          '(the reference always feeds full 256x512 inputs, backbone.py:80)')
            samples = samples.tensors
        elif isinstance(samples, (list, tuple)):
            samples = torch.stack(list(samples))
        # same hard shape contract as COTR/models/backbone.py:80
        assert samples.ndim == 4 and tuple(samples.shape[-2:]) == (MAX_SIZE, MAX_SIZE * 2) and samples.shape[1] == 3
        return samples

    @torch.no_grad()
    def encode(self, samples):
        """Query-independent half (backbone, input_proj, encoder, decoder K/V), cached in the
        HIP handle; follow with any number of ``decode(queries)``."""
        self._check_mode()
        img = self._as_batch(samples).contiguous().float()
        b = img.shape[0]
        self._call('cotr_encode', img.device, (b, 0), (img.data_ptr(), b), encoded=b)
        return self

    @torch.no_grad()
    def decode(self, queries):
        """pred_corrs [B,Q,2] for ``queries`` [B,Q,2] against the last ``encode``."""
        self._check_mode()
        b, q, two = queries.shape
        assert two == 2
        if self._encoded_batch != b:
            raise _lib.CotrHipError(f'decode of {b} pairs but the cached encode holds {self._encoded_batch}')
        qs = queries.contiguous().float()
        out = torch.empty((b, q, 2), dtype=torch.float32, device=qs.device)
        self._call('cotr_decode', qs.device, (b, q), (qs.data_ptr(), b, q, out.data_ptr()), keep_encode=True)
        return out

    @staticmethod
    def _varlen_offsets(counts, queries, pairs):
        """counts (host sequence of `pairs` non-negative ints summing to N, for packed queries [N, 2]) -> ctypes int[pairs + 1]
        offsets.  Raises ValueError before anything touches a device."""
        if queries.ndim != 2 or queries.shape[1] != 2:
            raise ValueError(f'varlen queries are packed [N, 2]; got {tuple(queries.shape)}')
        if isinstance(counts, torch.Tensor):
            if counts.is_floating_point() or counts.is_complex():
                raise ValueError('counts must be integers')
            counts = counts.tolist()
        counts = list(counts)
        if len(counts) != pairs:
            raise ValueError(f'{len(counts)} counts for {pairs} pairs')
        offsets = [0]
        for c in counts:
            if isinstance(c, bool) or int(c) != c or c < 0:
                raise ValueError(f'counts must be non-negative integers; got {c!r}')
            offsets.append(offsets[-1] + int(c))
        if offsets[-1] != queries.shape[0]:
            raise ValueError(f'counts sum to {offsets[-1]} but queries hold {queries.shape[0]} rows')
        if offsets[-1] >= 2 ** 31:
            raise ValueError(f'{offsets[-1]} query rows: the library indexes rows with int')
        return (ctypes.c_int * (pairs + 1))(*offsets)

    @torch.no_grad()
    def forward_varlen(self, samples, queries, counts):
        """A different number of queries per pair in one call: pair b owns the next counts[b] rows of the packed queries
        [N, 2] (device); returns the packed pred_corrs [N, 2] in the same order.  counts: host sequence of B non-negative
        ints summing to N.  Eval mode only.  Each row is what ``model(img[b:b+1], q_b[None])`` gives for it."""
        self._check_mode()
        img = self._as_batch(samples)
        b = img.shape[0]
        offsets = self._varlen_offsets(counts, queries, b)
        if img.device != queries.device:
            raise _lib.CotrHipError(f'samples on {img.device} but queries on {queries.device}')
        img = img.contiguous().float()
        qs = queries.contiguous().float()
        n = qs.shape[0]
        out = torch.empty((n, 2), dtype=torch.float32, device=img.device)
        self._call('cotr_forward_varlen', img.device, (b, -(-n // b)), (img.data_ptr(), qs.data_ptr(), offsets, b, out.data_ptr()),
                   encoded=b, varlen=True)
        return out

    @torch.no_grad()
    def decode_varlen(self, queries, counts):
        """forward_varlen's decode against the last ``encode`` (counts: one per encoded pair)."""
        self._check_mode()
        b = self._encoded_batch
        if b <= 0:
            raise _lib.CotrHipError('decode_varlen before encode')
        offsets = self._varlen_offsets(counts, queries, b)
        qs = queries.contiguous().float()
        n = qs.shape[0]
        out = torch.empty((n, 2), dtype=torch.float32, device=qs.device)
        self._call('cotr_decode_varlen', qs.device, (b, -(-n // b)), (qs.data_ptr(), offsets, b, out.data_ptr()),
                   keep_encode=True, varlen=True)
        return out

    @staticmethod
    def _pairs_args(images, pairs):
        """images [M, 3, 256, 256], pairs (host sequence of B (left, right) image indices, or an int tensor [B, 2]) -> (M, B, ctypes
        int[2B]).  Raises ValueError before anything touches a device.  A CUDA `pairs` tensor is copied to the host first: that copy
        waits for the work queued on its stream."""
        if not isinstance(images, torch.Tensor) or images.ndim != 4 or tuple(images.shape[1:]) != (3, MAX_SIZE, MAX_SIZE):
            raise ValueError(f'images must be [M, 3, {MAX_SIZE}, {MAX_SIZE}]; got {tuple(getattr(images, "shape", ()))}')
        m = images.shape[0]
        if m < 1:
            raise ValueError('images holds no image')
        if isinstance(pairs, torch.Tensor):
            if pairs.is_floating_point() or pairs.is_complex() or pairs.dtype == torch.bool:
                raise ValueError(f'pairs must be integers; got {pairs.dtype}')
            pairs = pairs.detach().cpu().tolist()
        try:
            rows = [list(p) for p in pairs]
        except TypeError:
            raise ValueError('pairs must be a sequence of (left, right) image indices') from None
        if not rows:
            raise ValueError('pairs holds no pair')
        flat = []
        for i, p in enumerate(rows):
            if len(p) != 2:
                raise ValueError(f'pair {i} has {len(p)} entries, not 2 (left, right)')
            for v in p:
                if isinstance(v, bool) or not isinstance(v, (int, np.integer)) or not 0 <= v < m:
                    raise ValueError(f'pair {i}: {v!r} is not an image index in [0, {m})')
                flat.append(int(v))
        return m, len(rows), (ctypes.c_int * len(flat))(*flat)

    @torch.no_grad()
    def encode_pairs(self, images, pairs):
        """encode() for B pairs drawn from M distinct images [M, 3, 256, 256] (each one half of a side-by-side input, normalised as
        for encode): pair b is (images[pairs[b][0]] | images[pairs[b][1]]).  Each image's backbone runs once.  Eval mode only;
        follow with decode(q) [B, Q, 2] or decode_varlen(q, counts).  Returns self."""
        self._check_mode()
        m, b, idx = self._pairs_args(images, pairs)
        imgs = images.contiguous().float()
        self._call('cotr_encode_pairs', imgs.device, (b, 0), (imgs.data_ptr(), m, idx, b), encoded=b, images=m)
        return self

    @torch.no_grad()
    def forward_pairs(self, images, pairs, queries):
        """forward() for B pairs drawn from M distinct images (see encode_pairs): queries [B, Q, 2] -> {'pred_corrs': [B, Q, 2]}, pair
        b's rows as ``model(torch.cat([images[l], images[r]], -1)[None], queries[b:b+1])`` gives them."""
        self._check_mode()
        m, b, idx = self._pairs_args(images, pairs)
        if queries.ndim != 3 or queries.shape[0] != b or queries.shape[2] != 2:
            raise ValueError(f'queries must be [{b}, Q, 2] for {b} pairs; got {tuple(queries.shape)}')
        if images.device != queries.device:
            raise _lib.CotrHipError(f'images on {images.device} but queries on {queries.device}')
        imgs = images.contiguous().float()
        qs = queries.contiguous().float()
        q = qs.shape[1]
        out = torch.empty((b, q, 2), dtype=torch.float32, device=imgs.device)
        self._call('cotr_forward_pairs', imgs.device, (b, q), (imgs.data_ptr(), m, idx, qs.data_ptr(), b, q, out.data_ptr()),
                   encoded=b, images=m)
        return {'pred_corrs': out}

    def pin_workspace(self, owner):
        """A captured HIP graph (training.GraphedTrainStep) holds the workspace's addresses: until unpin_workspace(owner) the
        workspace may not be replaced - a call that needs a larger one raises instead of silently freeing memory the graph writes."""
        self._workspace.pins.add(id(owner))

    def unpin_workspace(self, owner):
        self._workspace.pins.discard(id(owner))

    def reserve(self, pairs, queries):
        """Size the scratch workspace for calls of up to ``pairs`` x ``queries`` (optional; it otherwise grows on demand)."""
        dev = next(self.parameters()).device
        lib = self._ensure_ready(dev)
        with torch.cuda.device(dev):
            self._size_workspace(lib, dev, int(pairs), int(queries))

    @property
    def workspace(self):
        """The model's _Workspace (read-only: its buffer and the (pairs, queries) shape it serves)."""
        return self._workspace

    @property
    def _ws(self):      # workspace.buffer under the name it had as an attribute of the model: a plain alias, to read or to assign
        return self._workspace.buffer

    @_ws.setter
    def _ws(self, buffer):
        self._workspace.buffer = buffer

    def drop_workspace(self):
        """Forget the workspace and the cached encode: the next call sizes a new workspace - for that call alone, whatever varlen or
        pairs calls came before - and hands it over.  For callers that gave the handle a workspace of their own (cotr_set_workspace)."""
        if self._workspace.pins:
            raise _lib.CotrHipError('the workspace cannot be dropped while a captured training step (GraphedTrainStep) has its addresses '
                                    'baked in: close() the captured step first')
        self._workspace.release()
        self._workspace, self._encoded_batch = _Workspace(), 0

    def forward(self, samples, queries):
        if self.training:       # stage-1 training step: HIP backbone + HIP GEMMs under an autograd tape (training.py)
            from .. import training
            img = self._as_batch(samples)
            assert queries.ndim == 3 and queries.shape[2] == 2 and queries.shape[0] == img.shape[0]
            return {'pred_corrs': training.forward_train(self, img, queries)}
        return self._forward_eval(samples, queries)

    @torch.no_grad()
    def _forward_eval(self, samples, queries):
        img = self._as_batch(samples)
        b, q, two = queries.shape
        assert two == 2 and b == img.shape[0]
        if img.device != queries.device:
            raise _lib.CotrHipError(f'samples on {img.device} but queries on {queries.device}')
        img = img.contiguous().float()
        qs = queries.contiguous().float()
        out = torch.empty((b, q, 2), dtype=torch.float32, device=img.device)
        self._call('cotr_forward', img.device, (b, q), (img.data_ptr(), qs.data_ptr(), b, q, out.data_ptr()), encoded=b)
        return {'pred_corrs': out}

    @torch.no_grad()
    def backbone_upto(self, img, stage=3, out=None):
        """The frozen backbone through layer<stage> (1 ... 3) on the inference kernels (no gradient; the training step's frozen part):
        img [B, 3, 256, 512] -> [B, H, 2W, C] of that stage, NHWC over the side-by-side pair, written into `out` where one is given
        (float32, contiguous, on img's device, of exactly that shape)."""
        if stage not in (1, 2, 3):
            raise ValueError(f'stage must be 1, 2 or 3 (layer1 ... layer3); got {stage!r}')
        img = self._as_batch(img).detach().contiguous().float()
        b = img.shape[0]
        shape = (b, 128 >> stage, 256 >> stage, 128 << stage)
        if out is None:
            out = torch.empty(shape, dtype=torch.float32, device=img.device)
        elif tuple(out.shape) != shape or out.dtype != torch.float32 or out.device != img.device or not out.is_contiguous():
            raise ValueError(f'out must be a contiguous float32 tensor {shape} on {img.device}; got {out.dtype} {tuple(out.shape)} on '
                             f'{out.device}{"" if out.is_contiguous() else ", not contiguous"}')
        self._call('cotr_backbone_upto', img.device, (b, 1), (img.data_ptr(), b, stage, out.data_ptr()))
        return out

    # ------------------------------------------------------------------ tuning knobs (per handle: include/cotr_hip.h)
    def set_knob(self, name, value):
        """One tuning knob of this model's library handle (cotr_set_knob(h, ...)): other models - and other threads - keep theirs.
        Remembered, so it survives a move to another GPU; fusion thresholds / encode_chunk change the scratch the library needs,
        so the workspace is re-sized at the next call."""
        if self._workspace.pins:
            raise _lib.CotrHipError('tuning knobs change the carving of the workspace, and a captured training step (GraphedTrainStep) has '
                                    'its addresses baked in: set knobs before capturing, or close() the captured step first')
        if self._handle is not None:
            _lib.set_knob(name, value, self._handle)
        else:
            _lib.validate_knob(name, value)               # no handle yet: checked against the library's registry now, applied later
        self._knobs[name] = int(value)
        self._workspace.stale = True

    def knobs(self):
        """{name: (current, default)} of this model's handle (the shipped defaults + set_knob calls before the handle exists)."""
        if self._handle is not None:
            return _lib.knobs(self._handle)
        return {k: (self._knobs.get(k, v[1]), v[1]) for k, v in _lib.knobs(None).items()}

    def reset_knobs(self):
        if self._workspace.pins and self._knobs:
            raise _lib.CotrHipError('tuning knobs cannot change while a captured training step has the workspace pinned')
        if self._handle is not None:
            _lib.reset_knobs(self._handle)
        self._knobs = {}
        self._workspace.stale = True

    # ------------------------------------------------------------------ test / profiling hooks
    def debug_tap(self, name):
        lib = _lib.load_library()
        n = ctypes.c_size_t()
        _lib.check(lib.cotr_debug_tap(self._handle, name.encode(), None, 0, ctypes.byref(n), None), self._handle, 'tap')
        out = torch.empty(n.value, dtype=torch.float32, device=f'cuda:{self._handle_device}')
        _lib.check(lib.cotr_debug_tap(self._handle, name.encode(), out.data_ptr(), n.value, ctypes.byref(n),
                                      _lib.current_stream_ptr()), self._handle, 'tap')
        return out

    def set_debug_taps(self, enable=True):
        self._ensure_ready(next(self.parameters()).device)
        _lib.check(_lib.load_library().cotr_set_debug_taps(self._handle, int(enable)), self._handle, 'debug taps')

    def set_profiling(self, level=1):
        """0 off, 1 HIP-event timing per stage, 2 per kernel launch (see get_profile)."""
        self._ensure_ready(next(self.parameters()).device)
        _lib.check(_lib.load_library().cotr_set_profiling(self._handle, int(level)), self._handle, 'profiling')

    def _profile(self, with_ms):
        lib = _lib.load_library()
        cap, n = 256, ctypes.c_int(256)
        while n.value == cap:           # cotr_get_profile stops at the capacity and cannot report the total: full means ask again
            cap *= 2
            names, ms = (ctypes.c_char_p * cap)(), (ctypes.c_float * cap)() if with_ms else None
            _lib.check(lib.cotr_get_profile(self._handle, names, ms, cap, ctypes.byref(n)), self._handle, 'profile')
        return names[:n.value], ms[:n.value] if with_ms else None

    def get_profile(self):
        """[(name, ms)] of every entry of the last profiled call(s) since set_profiling."""
        names, ms = self._profile(True)
        return [(name.decode(), t) for name, t in zip(names, ms)]

    def profile_names(self):
        names, _ = self._profile(False)
        return [name.decode() for name in names]

    def batch_chunks(self, pairs, queries, which):
        """The passes a (pairs, queries) call is cut into under the model's knobs: pairs per pass; which = 0 encode, 1 decode."""
        lib = self._ensure_ready(next(self.parameters()).device)

        def ask(sizes, cap):
            n = lib.cotr_batch_chunks(self._handle, pairs, queries, which, sizes, cap)
            if n < 0:
                _lib.check(n, self._handle, 'cotr_batch_chunks')
            return n
        sizes = (ctypes.c_int * ask(None, 0))()     # the library reports the total whatever the capacity: the count first,
        if len(sizes):                              # then exactly that many slots
            ask(sizes, len(sizes))
        return list(sizes)


def build(args):
    return COTR(args)
