"""What the model and pipeline classes share, written once.

  PretrainedModel   the diffusers / transformers loading protocol (`from_config`, `from_pretrained`, `save_pretrained`), `dtype`,
                    `device` and the device guard of the six model classes (two UNets, two VAEs, two CLIP towers)
  GraphModel        what the two UNets add: `invalidate_caches` on every way the weights can change, `enable_graph`, the session
                    store and the batched small projections
  Session           static input buffers of one input signature; with graphs enabled, warm-up, capture and replay
  PretrainedPipeline  `save_pretrained` / `to` of the two pipeline families, `read_scheduler_config`

The literal names a class writes into its files (`class_name`, `config_extra`) are attributes of the class that defines them, so a
subclass keeps writing its parent's name.
"""
from __future__ import annotations

import gc
import inspect
import json
import os

import torch
import torch.nn as nn

from . import _lib, ops
from .layers import weights_key


def require_device(x, name):
    if not x.is_cuda and not _lib.host_pointers_ok():
        raise RuntimeError(f"animate_anything_amd.{name} runs on the GPU only (no CPU fallback)")


class PretrainedModel(nn.Module):
    config_name = "config.json"
    class_name = None                          # the name in the device guard's message
    config_extra = {}                          # entries of config.json beyond vars(self.config)
    config_section = None                      # nested section of a composite config.json, folded in under the top level
    weights_name = "diffusion_pytorch_model"   # <weights_name>.safetensors, read and written
    weights_bin_name = None                    # <weights_bin_name>.bin, read only (None: weights_name)

    @property
    def dtype(self):
        return next(self.parameters()).dtype

    @property
    def device(self):
        return next(self.parameters()).device

    def require_device(self, x):
        require_device(x, self.class_name)

    @classmethod
    def from_config(cls, config: dict, **overrides):
        cfg = {k: v for k, v in dict(config).items() if not k.startswith("_")}
        if cls.config_section is not None:
            cfg = dict(cfg.get(cls.config_section) or {}, **{k: v for k, v in cfg.items() if k != cls.config_section})
        cfg.update(overrides)
        ok = set(inspect.signature(cls.__init__).parameters) - {"self"}
        return cls(**{k: v for k, v in cfg.items() if k in ok})

    @classmethod
    def from_pretrained(cls, path, subfolder=None, torch_dtype=None, variant=None, **overrides):
        """Load a diffusers / transformers directory: config.json + <weights_name>.safetensors / <weights_bin_name>.bin."""
        root = os.path.join(path, subfolder) if subfolder else path
        with open(os.path.join(root, cls.config_name)) as f:
            model = cls.from_config(json.load(f), **overrides)
        from ._ckpt import load_state
        model.load_state_dict(load_state(root, cls.weights_name, variant, cls.weights_bin_name))
        return model.to(torch_dtype) if torch_dtype is not None else model

    def save_pretrained(self, path):
        os.makedirs(path, exist_ok=True)
        with open(os.path.join(path, self.config_name), "w") as f:
            json.dump(dict(vars(self.config), **self.config_extra), f, indent=2)
        from safetensors.torch import save_file
        save_file({k: v.contiguous().cpu() for k, v in self.state_dict().items()},
                  os.path.join(path, self.weights_name + ".safetensors"))


class GraphModel(PretrainedModel):
    _packs = ("_temb_pack", "_text_pack")      # derived copies of the weights that `invalidate_caches` drops

    def _apply(self, fn, *a, **k):
        self.invalidate_caches()
        return super()._apply(fn, *a, **k)

    def load_state_dict(self, *a, **k):
        out = super().load_state_dict(*a, **k)
        self.invalidate_caches()
        return out

    def invalidate_caches(self):
        """Drop every derived copy of the weights: the batched time-embedding / text K|V packs and the captured hipGraphs
        (which replay launches that point at the packed copies).  Called on `.to()` / `load_state_dict()`; call it by hand
        after editing parameters in place while a graph is enabled (the per-layer packs notice in-place edits themselves,
        a captured graph cannot)."""
        for name in self._packs:
            setattr(self, name, None)
        if getattr(self, "_graph", None) is not None:
            self._graph = {}

    def enable_graph(self, enabled=True):
        """Capture the forward (embeddings + input packing + `_core`) in a hipGraph on first use per input signature and
        replay it afterwards (removes ~1k host launches per denoising step)."""
        self._graph = {} if enabled else None

    def _session(self, key, device, make):
        """The session of `key`, made by `make(self, key, device)` on first use: one per key with graphs enabled, else one at all."""
        store = self._graph if self._graph is not None else self.__dict__.setdefault("_eager_sessions", {})
        sess = store.get(key)
        if sess is None:
            if self._graph is None:
                store.clear()                                  # eager sessions hold only input buffers: keep one
            sess = store[key] = make(self, key, device)
        return sess

    def _project_batched(self, x, pack, pick, linears, attr):
        """Many small projections of the same rows as ONE contraction (each alone is a latency-bound launch): the weight rows
        (and biases) of `linears(m)` of every module `m` with `pick(m)`, in `self.modules()` order, concatenated and packed under
        the attribute `pack`; every module receives its column slice of the result as `m.<attr>`."""
        mods = self.__dict__.get(pack + "_modules")
        if mods is None:
            mods = self.__dict__[pack + "_modules"] = [m for m in self.modules() if pick(m)]
        lins = [linears(m) for m in mods]
        key = weights_key(*[t for ls in lins for l in ls for t in (l.weight, l.bias)])
        cached = getattr(self, pack, None)
        if cached is None or cached[0] != key:
            flat = [l for ls in lins for l in ls]
            w = torch.cat([l.weight.detach() for l in flat], dim=0)
            bias = None if flat[0].bias is None else torch.cat([l.bias.detach() for l in flat], dim=0)
            offs = [0]
            for ls in lins:
                offs.append(offs[-1] + sum(l.weight.shape[0] for l in ls))
            cached = (key, ops.pack_weight(w, bias), mods, offs)
            setattr(self, pack, cached)
        _, pw, mods, offs = cached
        proj = ops.conv_gemm(x, pw, ops.linear_geom(x.shape[0]))                           # [rows, sum of the widths]
        for i, m in enumerate(mods):
            setattr(m, attr, proj[:, offs[i]:offs[i + 1]])


class Session:
    """Static input buffers of one input signature of a GraphModel (`inputs`); a caller that owns the denoising loop writes its
    inputs straight into them once and then only calls `run()` per step.  A subclass allocates `inputs` and says in `_core()` how
    they reach `net._core`."""

    def __init__(self, net):
        self.net = net
        self.graph = None
        self.out = None

    def load(self, **tensors):
        for k, v in tensors.items():
            dst = self.inputs[k]
            if dst is not None and v is not None and dst.data_ptr() != v.data_ptr():
                dst.copy_(v.reshape(dst.shape) if v.numel() == dst.numel() else v.expand(dst.shape))

    def run(self):
        if self.net._graph is None:
            return self._core()
        if self.graph is None:
            s = torch.cuda.Stream()
            s.wait_stream(torch.cuda.current_stream())
            with torch.cuda.stream(s):                                   # warm-up outside capture (packs weights, autotunes)
                self._core()
            torch.cuda.current_stream().wait_stream(s)
            self.graph = torch.cuda.CUDAGraph()
            # A model and its sessions refer to each other, so a dropped model is released by the cycle collector, whenever that
            # runs - and releasing hipGraphs and device memory in the middle of a capture aborts the process.  Collect now, and
            # keep the collector out of the capture (torch.cuda.graph itself no longer collects on entry).
            gc.collect()
            collecting = gc.isenabled()
            gc.disable()
            try:
                with torch.cuda.graph(self.graph):
                    self.out = self._core()
            finally:
                if collecting:
                    gc.enable()
        self.graph.replay()
        return self.out


def read_scheduler_config(path):
    """`scheduler/scheduler_config.json` of a diffusers pipeline directory, {} when absent."""
    cfg_path = os.path.join(path, "scheduler", "scheduler_config.json")
    if not os.path.exists(cfg_path):
        return {}
    with open(cfg_path) as f:
        return json.load(f)


class PretrainedPipeline:
    class_name = None                          # `_class_name` of model_index.json
    components = ()                            # saved through their own `save_pretrained` when present
    on_device = ()                             # the components `to` moves

    def save_pretrained(self, path):
        """diffusers directory layout (what `from_pretrained` reads): one directory per component that is present and can save
        itself, scheduler/scheduler_config.json, model_index.json."""
        os.makedirs(path, exist_ok=True)
        index = {"_class_name": self.class_name}
        for name in self.components:
            m = getattr(self, name)
            if m is not None and hasattr(m, "save_pretrained"):
                m.save_pretrained(os.path.join(path, name))
                index[name] = [type(m).__module__.split(".")[0], type(m).__name__]
        os.makedirs(os.path.join(path, "scheduler"), exist_ok=True)
        with open(os.path.join(path, "scheduler", "scheduler_config.json"), "w") as f:
            json.dump(dict(vars(self.scheduler.config), _class_name=type(self.scheduler).__name__), f, indent=2)
        index["scheduler"] = ["animate_anything_amd", type(self.scheduler).__name__]
        with open(os.path.join(path, "model_index.json"), "w") as f:
            json.dump(index, f, indent=2)

    def to(self, device=None, torch_dtype=None, **_):
        for name in self.on_device:
            m = getattr(self, name)
            if m is not None:
                if device is not None:
                    m.to(device)
                if torch_dtype is not None:
                    m.to(torch_dtype)
        return self
