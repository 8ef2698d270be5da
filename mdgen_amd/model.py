"""`LatentMDGenModel` -- drop-in for `mdgen.model.latent_model.LatentMDGenModel` (inference path).

`forward` / `forward_inference` keep the reference signature (latent_model.py:212-216, 263-269) and
dispatch to `mdgen_denoiser_forward`; `sample_euler` runs the whole S-step Euler rollout
(`mdgen_sample_euler`, optionally replayed from a hipGraph).  All arithmetic is in libmdgen_amd.so;
this class owns the opaque context, the workspaces and persistent staging buffers (stable pointers
are what make hipGraph replay possible).
"""
from __future__ import annotations

import contextlib
import ctypes as C
from collections import OrderedDict
from typing import Dict, Optional

import torch

from . import _lib as L
from ._lib import lib, check, ptr, require_cuda
from .config import ModelConfig
from .rigid_utils import Rigid


def _frames(fr):
    """Rigid | (rot, trans) | None -> (rot [B,L,3,3], trans [B,L,3]) contiguous fp32."""
    if fr is None:
        return None, None
    if isinstance(fr, Rigid):
        r, t = fr.get_rots().get_rot_mats(), fr.get_trans()
    else:
        r, t = fr
    return r.to(torch.float32).contiguous(), t.to(torch.float32).contiguous()


class LatentMDGenModel:
    def __init__(self, cfg: ModelConfig, device: Optional[torch.device] = None, precision: str = "bf16"):
        """`precision`: "bf16" (default) -- bf16 MFMA operands, fp32 accumulate / softmax / LayerNorm / residual stream;
        "fp32" -- the reference's own arithmetic on fp32 operands (csrc/k_fp32.hip), a tolerance mode ~10x slower.
        A model built with "fp32" keeps fp32 weight copies and can switch at run time (`set_precision`)."""
        if isinstance(cfg, ModelConfig) is False:
            cfg = ModelConfig.from_args(cfg)
        if precision not in ("bf16", "fp32"):
            raise L.MdgenError(f"precision must be 'bf16' or 'fp32', got {precision!r}")
        self.cfg = cfg
        self.precision = precision
        self.device = torch.device(device if device is not None else "cuda")
        if self.device.type != "cuda" or not torch.cuda.is_available():
            raise L.MdgenError("mdgen_amd.LatentMDGenModel needs a GPU (gfx950); there is no CPU path")
        d = L.ModelDesc(cfg.embed_dim, cfg.mha_heads, cfg.num_layers, cfg.latent_dim, cfg.ipa_heads,
                        cfg.ipa_head_dim, cfg.ipa_qk, cfg.ipa_v, int(cfg.abs_pos_emb), cfg.crop,
                        int(cfg.tps_condition), float(cfg.time_multiplier))
        self._ctx = C.c_void_p()
        with torch.cuda.device(self.device):
            check(lib.mdgen_ctx_create(C.byref(self._ctx), C.byref(d)))
        if precision == "fp32":
            check(lib.mdgen_ctx_set_option(self._ctx, b"keep_fp32_weights", 1))
        # small LRU caches, keyed independently: a workspace per (B, T, L, S, t_shared) and the persistent staging
        # buffers of the Euler rollout per (B, T, L) -- stable device pointers are what lets a captured hipGraph be
        # replayed, so alternating shapes (ATLAS inference runs on full sequences, L = 39..724) or alternating
        # forward() / sample_euler() calls must not evict each other's buffers on every call.
        self._ws: "OrderedDict[tuple, torch.Tensor]" = OrderedDict()
        self._stage: "OrderedDict[tuple, dict]" = OrderedDict()
        self.max_cached_shapes = 4
        self.poison_workspace = False     # tests: fill new workspaces with 0xFF (NaN in fp32 and bf16)
        self._side = None
        self._loaded = False
        self._pre_run = None              # optional hook run before every network evaluation (train.TrainableModel: lazy weight refresh)

    def __del__(self):
        try:
            if getattr(self, "_ctx", None):
                lib.mdgen_ctx_destroy(self._ctx)
                self._ctx = None
        except Exception:
            pass

    # ---- weights ----------------------------------------------------------------------------
    def weight_names(self):
        n = lib.mdgen_ctx_num_weights(self._ctx)
        return [lib.mdgen_ctx_weight_name(self._ctx, i).decode() for i in range(n)]

    def load_state_dict(self, sd, strict: bool = True):
        """`sd`: the reference's `LatentMDGenModel.state_dict()` (keys of SURVEY.md section 8(b))."""
        names = set(self.weight_names())
        missing = [k for k in names if k not in sd]
        unexpected = [k for k in sd if k not in names]
        if strict and (missing or unexpected):
            raise L.MdgenError(f"state_dict mismatch: missing={missing[:5]} unexpected={unexpected[:5]}")
        keep = []
        with torch.cuda.device(self.device):
            s = L.stream_ptr()
            for k in names:
                if k not in sd:
                    continue
                t = sd[k].detach().to(device=self.device, dtype=torch.float32).contiguous()
                keep.append(t)
                shp = (C.c_int64 * t.dim())(*t.shape)
                check(lib.mdgen_ctx_set_weight(self._ctx, k.encode(), ptr(t), shp, t.dim(), s))
            check(lib.mdgen_ctx_finalize(self._ctx, s))
            torch.cuda.current_stream().synchronize()   # packing kernels read `keep` asynchronously
        self._loaded = True
        self._state_names = list(sd.keys())
        if self.precision == "fp32":
            self.set_precision("fp32")
        return self

    def set_precision(self, precision: str):
        """Switch between the bf16 MFMA path and the fp32 path (the latter only on a model constructed with
        precision="fp32", which keeps the fp32 weight copies)."""
        if precision not in ("bf16", "fp32"):
            raise L.MdgenError(f"precision must be 'bf16' or 'fp32', got {precision!r}")
        check(lib.mdgen_ctx_set_option(self._ctx, b"precision", 32 if precision == "fp32" else 16))
        self.precision = precision
        return self

    def eval(self):
        return self

    def to(self, device):
        if torch.device(device).type != "cuda":
            raise L.MdgenError("mdgen_amd has no CPU path")
        return self

    def set_option(self, name: str, value: int):
        """Library run-time options (include/mdgen_amd.h `mdgen_ctx_set_option`), e.g. "streams", "precision",
        "keep_fp32_weights", "attention_path", "mlp_path", "residue_l4_path" (2 one kernel | 1 | 0 general path), "fuse_proj"
        (3 panel MLP prologue | 0 off).  An unknown name or a value the library does not accept raises MdgenError."""
        check(lib.mdgen_ctx_set_option(self._ctx, name.encode(), int(value)))
        return self

    # ---- measurement ------------------------------------------------------------------------
    def profile(self, on: bool):
        check(lib.mdgen_profile_enable(self._ctx, int(on)))

    def phase_trace(self, buf):
        """Arm the one-shot phase trace: the next trunk MLP launch writes [wave][32] s_memtime stamps into the
        int64 CUDA tensor `buf` (None cancels).  Measurement only; use with use_graph=False."""
        if buf is None:
            check(lib.mdgen_profile_phase_trace(self._ctx, None, 0))
        else:
            assert buf.is_cuda and buf.dtype == torch.int64 and buf.is_contiguous()
            check(lib.mdgen_profile_phase_trace(self._ctx, buf.data_ptr(), buf.numel()))

    def profile_report(self) -> dict:
        """{"kernel class": {"count": n, "ms": total}} measured with hipEvents on the launch stream."""
        import json
        buf = C.create_string_buffer(1 << 16)
        with torch.cuda.device(self.device):
            check(lib.mdgen_profile_report(self._ctx, L.stream_ptr(), buf, len(buf)))
        rep = json.loads(buf.value.decode())
        # "@context" is not a kernel class: the placement-probe result (xcd_round_robin), the CU count and the number of
        # split-panel launches (k_mlp8<., 3>) since the last report
        self.context_info = rep.pop("@context", None)
        return rep

    # ---- workspace --------------------------------------------------------------------------
    def graph_count(self) -> int:
        """`mdgen_debug_graph_count`: the captured hipGraphs the context holds."""
        n = C.c_int32()
        check(lib.mdgen_debug_graph_count(self._ctx, C.byref(n)))
        return n.value

    def workspace_layout(self, B, T, L_, S, t_shared):
        lay = L.WsLayout()
        sh = L.Shape(B, T, L_)
        check(lib.mdgen_workspace_layout(self._ctx, C.byref(sh), S, int(t_shared), C.byref(lay)))
        return lay

    def _cached(self, cache, key, make, stale=None):
        """LRU get-or-create over `self._ws` / `self._stage` (at most max_cached_shapes entries each); an entry that `stale`
        names is dropped and made again."""
        v = cache.get(key)
        if v is not None and stale is not None and stale(v):
            del cache[key]
            v = None
        if v is None:
            while len(cache) >= self.max_cached_shapes:
                cache.popitem(last=False)                     # least recently used
            v = cache[key] = make()
        else:
            cache.move_to_end(key)
        return v

    def _sized_workspace(self, key, nbytes):
        """The workspace cached under `key`, of at least `nbytes` bytes."""
        def make():
            ws = torch.empty(nbytes, dtype=torch.uint8, device=self.device)
            if self.poison_workspace:
                ws.fill_(255)
            return ws
        return self._cached(self._ws, key, make, lambda ws: ws.numel() < nbytes)

    def _workspace(self, B, T, L_, S, t_shared):
        lay = self.workspace_layout(B, T, L_, S, t_shared)   # (options may have changed what the call needs: mlp_fold, precision)
        return self._sized_workspace((B, T, L_, S, int(t_shared)), lay.total_bytes)

    @contextlib.contextmanager
    def _call_stream(self, use_graph: bool):
        """Makes the model's device current and yields the hipStream_t a library call goes on: the current stream, or -- with
        `use_graph`, since a capture needs a non-default stream -- the model's side stream, ordered after the current stream on entry
        and ahead of it on exit."""
        with torch.cuda.device(self.device):
            cur = torch.cuda.current_stream()
            if not use_graph:
                yield C.c_void_p(cur.cuda_stream)
                return
            if self._side is None:
                self._side = torch.cuda.Stream(device=self.device)
            self._side.wait_stream(cur)
            yield C.c_void_p(self._side.cuda_stream)
            cur.wait_stream(self._side)

    # ---- forward ----------------------------------------------------------------------------
    def _check_inputs(self, x, mask, x_cond, x_cond_mask, aatype):
        if x_cond is None or x_cond_mask is None or aatype is None:
            raise L.MdgenError("x_cond, x_cond_mask and aatype are required (conditional models only)")
        if x.dim() != 4 or x.shape[-1] != self.cfg.latent_dim:
            raise L.MdgenError(f"x must be (B,T,L,{self.cfg.latent_dim}), got {tuple(x.shape)}")
        B, T, L_, _ = x.shape
        if tuple(mask.shape) != (B, T, L_):
            raise L.MdgenError(f"mask must be (B,T,L)={B, T, L_}, got {tuple(mask.shape)}")
        return B, T, L_

    def _rel7(self, rel_quats, B, L_):
        """Optional relative-frame inputs of the two-sided model, (2,B,L,7): [0] = (start^-1 o end).to_tensor_7(), [1] =
        (end^-1 o start).to_tensor_7() (latent_model.py:193-195) as the CALLER's reference computed them -- their quaternion
        sign is torch.linalg.eigh's (rigid_utils.py:191-210).  None: the library computes them with w >= 0."""
        if rel_quats is None:
            return None
        if not self.cfg.tps_condition:
            raise L.MdgenError("rel_quats is an input of tps_condition models only")
        if tuple(rel_quats.shape) != (2, B, L_, 7):
            raise L.MdgenError(f"rel_quats must be (2,B,L,7)={(2, B, L_, 7)}, got {tuple(rel_quats.shape)}")
        require_cuda(rel_quats)
        return rel_quats.to(torch.float32).contiguous()

    def forward(self, x, t, mask, start_frames=None, end_frames=None, x_cond=None, x_cond_mask=None, aatype=None,
                return_trace: bool = False, rel_quats=None):
        """latent_model.py:212-260 (non-design path).  Returns the velocity (B,T,L,D) fp32."""
        if self._pre_run is not None:
            self._pre_run()
        B, T, L_ = self._check_inputs(x, mask, x_cond, x_cond_mask, aatype)
        require_cuda(x, t, mask, x_cond, x_cond_mask, aatype)
        sr, st = _frames(start_frames)
        er, et = _frames(end_frames)
        if sr is None:
            raise L.MdgenError("start_frames is required (prepend_ipa models)")
        x = x.to(torch.float32).contiguous()
        t = t.to(torch.float32).contiguous()
        mask = mask.to(torch.float32).contiguous()
        x_cond = x_cond.to(torch.float32).contiguous()
        x_cond_mask = x_cond_mask.to(torch.int64).contiguous()
        aatype = aatype.to(torch.int64).contiguous()
        out = torch.empty_like(x)
        ws = self._workspace(B, T, L_, 1, B == 1)
        nl = self.cfg.num_layers
        tr_h = torch.empty(nl + 1, B * T * L_, self.cfg.embed_dim, device=x.device) if return_trace else None
        tr_i = torch.empty(B * L_, self.cfg.embed_dim, device=x.device) if return_trace else None
        sh = L.Shape(B, T, L_)
        rel7 = self._rel7(rel_quats, B, L_)
        cond = L.cond(mask, sr, st, er, et, rel7, x_cond, x_cond_mask, aatype)
        with self._call_stream(False) as stream:
            check(lib.mdgen_denoiser_forward(self._ctx, C.byref(sh), ptr(x), ptr(t), C.byref(cond), ptr(out), ptr(tr_h), ptr(tr_i),
                                             ptr(ws), ws.numel(), stream))
        if return_trace:
            C_ = self.cfg.embed_dim
            trace = {"ipa_out": tr_i.view(B, L_, C_)}
            for i in range(nl + 1):
                trace[f"h{i}"] = tr_h[i].view(B, T, L_, C_)
            return out, trace
        return out

    forward_inference = forward
    __call__ = forward

    # ---- samplers ---------------------------------------------------------------------------
    def _sampler_inputs(self, zs, mask, start_frames, end_frames, x_cond, x_cond_mask, aatype):
        """The checks every conditioned sampler starts with -> (B, T, L, start rot, start trans, end rot | None, end trans | None)."""
        if self._pre_run is not None:
            self._pre_run()
        B, T, L_ = self._check_inputs(zs, mask, x_cond, x_cond_mask, aatype)
        require_cuda(zs, mask, x_cond, x_cond_mask, aatype)
        sr, st = _frames(start_frames)
        if sr is None:
            raise L.MdgenError("start_frames is required")
        return (B, T, L_, sr, st) + _frames(end_frames)

    def _staged(self, key, spec: dict, given: dict):
        """The persistent staging set under `key` (stable device pointers => hipGraph replay): a buffer per name: (shape, dtype) of
        `spec`, with the tensors of `given` copied into theirs (None: that buffer is left as it is)."""
        stg = self._cached(self._stage, key, lambda: {
            n: torch.empty(shape, dtype=dt, device=self.device) for n, (shape, dt) in spec.items()})
        for n, t in given.items():
            if t is not None:
                stg[n].copy_(t)
        return stg

    def _stage_cond(self, zs, mask, sr, st, er, et, x_cond, x_cond_mask, aatype, rel_quats):
        """Stages a call's state and conditioning in the buffers of its shape, one set for sample_euler and sample_rk
        -> (the state buffer, the `L.Cond` of the others; NULL where the call gives none)."""
        B, T, L_, D = zs.shape
        f32, i64 = torch.float32, torch.int64
        spec = dict(x=((B, T, L_, D), f32), mask=((B, T, L_), f32), sr=((B, L_, 3, 3), f32), st=((B, L_, 3), f32),
                    er=((B, L_, 3, 3), f32), et=((B, L_, 3), f32), x_cond=((B, T, L_, D), f32), x_cond_mask=((B, T, L_), i64),
                    aatype=((B, L_), i64))
        if self.cfg.tps_condition:
            spec["rel7"] = ((2, B, L_, 7), f32)
        given = dict(mask=mask, sr=sr, st=st, er=er, et=et, rel7=self._rel7(rel_quats, B, L_), x_cond=x_cond,
                     x_cond_mask=x_cond_mask, aatype=aatype)   # (in the order of L.Cond's fields)
        stg = self._staged((B, T, L_), spec, dict(given, x=zs))
        return stg["x"], L.cond(*[stg[n] if t is not None else None for n, t in given.items()])

    def sample_euler(self, zs, num_steps: int, mask=None, start_frames=None, end_frames=None, x_cond=None,
                     x_cond_mask=None, aatype=None, use_graph: bool = True, rel_quats=None):
        """x <- zs; for i < S: x += (t[i+1]-t[i]) * model(x, t[i]) on t = linspace(0,1,S+1); returns x.
        (transport.py:408-451 + integrators.py:95-114 + torchdiffeq fixed-grid Euler.)"""
        B, T, L_, *frames = self._sampler_inputs(zs, mask, start_frames, end_frames, x_cond, x_cond_mask, aatype)
        S = int(num_steps)
        ws = self._workspace(B, T, L_, S, True)
        x, cond = self._stage_cond(zs, mask, *frames, x_cond, x_cond_mask, aatype, rel_quats)
        sh = L.Shape(B, T, L_)
        with self._call_stream(use_graph) as stream:
            check(lib.mdgen_sample_euler(self._ctx, C.byref(sh), S, ptr(x), C.byref(cond), ptr(ws), ws.numel(), int(use_graph), stream))
        return x.clone()

    # ---- adaptive dopri5 ----------------------------------------------------------------------
    def sample_dopri5(self, zs, mask=None, start_frames=None, end_frames=None, x_cond=None, x_cond_mask=None, aatype=None,
                      atol: float = 1e-6, rtol: float = 1e-3, rel_quats=None, max_steps: int = 10000):
        """The reference's default solver (`mdgen_sample_dopri5`): torchdiffeq 0.2.x odeint(model, zs, linspace(0, 1, 50),
        method='dopri5', atol=[atol], rtol=[rtol])[-1] (transport.py:408-451, integrators.py:74-113).  One step size for the
        whole batch (the error norm spans every element).  Returns (x at t = 1, stats) with stats = {"nfe", "accepted",
        "rejected", "steps": [(t0, dt) of every accepted step]}.  Synchronises the current stream once per attempted step."""
        B, T, L_, sr, st, er, et = self._sampler_inputs(zs, mask, start_frames, end_frames, x_cond, x_cond_mask, aatype)
        sh = L.Shape(B, T, L_)
        nbytes = C.c_size_t()
        check(lib.mdgen_dopri5_workspace_bytes(self._ctx, C.byref(sh), C.byref(nbytes)))
        ws = self._sized_workspace(("dopri5", B, T, L_), nbytes.value)
        x = zs.to(torch.float32).contiguous().clone()
        mask = mask.to(torch.float32).contiguous()
        x_cond = x_cond.to(torch.float32).contiguous()
        x_cond_mask = x_cond_mask.to(torch.int64).contiguous()
        aatype = aatype.to(torch.int64).contiguous()
        cond = L.cond(mask, sr, st, er, et, self._rel7(rel_quats, B, L_), x_cond, x_cond_mask, aatype)
        stats = (C.c_int32 * 3)()
        steps = (C.c_double * (2 * int(max_steps)))()
        with self._call_stream(False) as stream:
            check(lib.mdgen_sample_dopri5(self._ctx, C.byref(sh), float(atol), float(rtol), int(max_steps), ptr(x), C.byref(cond),
                                          ptr(ws), ws.numel(), stats, steps, stream))
        acc = stats[1]
        info = {"nfe": stats[0], "accepted": acc, "rejected": stats[2],
                "steps": [(steps[2 * i], steps[2 * i + 1]) for i in range(acc)]}
        return x, info

    # ---- fixed-grid Runge-Kutta ---------------------------------------------------------------
    def sample_rk(self, zs, method: str, num_steps: int, mask=None, start_frames=None, end_frames=None, x_cond=None,
                  x_cond_mask=None, aatype=None, use_graph: bool = True, rel_quats=None):
        """`mdgen_sample_rk`: `method` in ("midpoint", "heun3", "rk4") with one step per interval of t = linspace(0, 1, S + 1),
        S = `num_steps` (torchdiffeq 0.2.x fixed-grid solvers as transport.py:408-451 / integrators.py:106-113 call them): 2, 3, 4
        network evaluations per step.  Every sample sees the same grid, so a sample's solution does not depend on its batch mates;
        nothing synchronises, and with `use_graph` the whole solve is one hipGraph.  Returns x at t = 1."""
        B, T, L_, *frames = self._sampler_inputs(zs, mask, start_frames, end_frames, x_cond, x_cond_mask, aatype)
        (code, S), ws = self._rk_call(method, num_steps, B, T, L_)
        sh = L.Shape(B, T, L_)
        x, cond = self._stage_cond(zs, mask, *frames, x_cond, x_cond_mask, aatype, rel_quats)
        with self._call_stream(use_graph) as stream:
            check(lib.mdgen_sample_rk(self._ctx, C.byref(sh), code, S, ptr(x), C.byref(cond), ptr(ws), ws.numel(), int(use_graph), stream))
        return x.clone()

    # ---- SDE: Euler-Maruyama / Heun --------------------------------------------------------------
    def sample_sde(self, zs, opts, mask=None, start_frames=None, end_frames=None, x_cond=None, x_cond_mask=None, aatype=None,
                   noise=None, use_graph: bool = True, rel_quats=None, noise_step_stride=None, rng=None):
        """`mdgen_sample_sde`: the reference's `Sampler.sample_sde` (transport.py:295-406) with `opts` = `_lib.sde_opts(
        sampling_method, path_type, diffusion_form, diffusion_norm, last_step, last_step_size, num_steps, sample_eps)`:
        n_points - 1 Euler-Maruyama or Heun steps on linspace(t0, t1, n_points), then the last step; n_points - 1 or
        2 (n_points - 1) network evaluations, one more with a last step.  Nothing synchronises, and with `use_graph` the whole
        solve is one hipGraph.  `noise`: (n_points - 1, B, T, L, D) standard normals, one tensor per step; None: drawn with
        torch.randn from the device generator, so the same torch.manual_seed gives the same sample.  The noise is staged in a
        persistent buffer of (n_points - 1) x state bytes (stable pointers: the graph is replayed with new noise in it) -- at
        250 points and B 16 x T 1000 x L 4 that is 1.3 GB.  `noise_step_stride` (floats, a multiple of 4, at least one state;
        default: one state rounded up to 4) is the distance between two steps' noise in that buffer.
        `rng`: a device int64 tensor of four words {seed, sample_base, block_base, 0} (`_lib.rng_words`) in the noise's place
        (`mdgen_sample_sde_rng`): the kernels generate the noise from it (Philox, include/mdgen_amd.h) and nothing is staged; the
        words are read on the device, so write them on the current stream before the call and keep the tensor for replays.
        Returns the sample."""
        B, T, L_, *frames = self._sampler_inputs(zs, mask, start_frames, end_frames, x_cond, x_cond_mask, aatype)
        D, S = zs.shape[-1], opts.n_points - 1
        sh = L.Shape(B, T, L_)
        ws = self._sde_workspace(opts, B, T, L_)
        if rng is not None:
            if noise is not None or noise_step_stride is not None:
                raise L.MdgenError("rng generates the noise in the kernels: it goes without noise / noise_step_stride")
            self._check_rng(rng)
            x, cond = self._stage_cond(zs, mask, *frames, x_cond, x_cond_mask, aatype, rel_quats)
            with self._call_stream(use_graph) as stream:
                check(lib.mdgen_sample_sde_rng(self._ctx, C.byref(sh), C.byref(opts), ptr(x), ptr(rng), C.byref(cond), ptr(ws), ws.numel(),
                                               int(use_graph), stream))
            return x.clone()
        state = B * T * L_ * D
        stride = (state + 3) // 4 * 4 if noise_step_stride is None else int(noise_step_stride)
        if stride < state:
            raise L.MdgenError(f"noise_step_stride {stride} is below one state of {state} floats")
        if noise is not None and tuple(noise.shape) != (S, B, T, L_, D):
            raise L.MdgenError(f"noise must be (n_points - 1, B, T, L, D) = {(S, B, T, L_, D)}, got {tuple(noise.shape)}")
        x, cond = self._stage_cond(zs, mask, *frames, x_cond, x_cond_mask, aatype, rel_quats)
        buf = self._staged(("sde_noise", S, stride), dict(noise=((S, stride), torch.float32)), {})["noise"]
        if noise is None:
            noise = torch.randn(S, B, T, L_, D, device=self.device)
        require_cuda(noise)
        buf[:, :state].copy_(noise.reshape(S, state))
        with self._call_stream(use_graph) as stream:
            check(lib.mdgen_sample_sde(self._ctx, C.byref(sh), C.byref(opts), ptr(x), ptr(buf), stride, C.byref(cond), ptr(ws), ws.numel(),
                                       int(use_graph), stream))
        return x.clone()

    def _sde_workspace(self, opts, B, T, L_):
        """The workspace of an SDE call of this shape (`mdgen_sde_workspace_bytes` refuses bad options first): one for sample_sde
        and the drivers."""
        sh = L.Shape(B, T, L_)
        nbytes = C.c_size_t()
        check(lib.mdgen_sde_workspace_bytes(self._ctx, C.byref(sh), C.byref(opts), C.byref(nbytes)))
        return self._sized_workspace(("sde", B, T, L_), nbytes.value)

    def _check_rng(self, rng):
        require_cuda(rng)
        if rng.dtype != torch.int64 or tuple(rng.shape) != (4,) or not rng.is_contiguous():
            raise L.MdgenError("rng must be a contiguous device int64 tensor of four words (_lib.rng_words)")

    # ---- multi-block rollout -----------------------------------------------------------------
    def rollout_euler(self, zs, num_steps: int, mask, cond_rots, cond_trans, cond_torsions, seqres, tables,
                      use_graph: bool = True):
        """`mdgen_rollout_euler`: R = zs.shape[0] chained T-frame blocks in one call (one hipGraph), the driver loop
        of sim_inference.py:100-113.  zs (R,B,T,L,D) noise; mask (B,T,L); cond_* the first conditioning frame
        (B,L,...); seqres (B,L) int64; tables: dict of residue tables on the device (geometry.residue_tables).
        Returns (atom14 (B, R*T, L, 14, 3), samples (R,B,T,L,D), next conditioning frame dict)."""
        S = int(num_steps)
        return self._rollout("rollout", lib.mdgen_rollout_euler, lambda *shape: ((S,), self._workspace(*shape, S, True)), False,
                             zs, mask, cond_rots, cond_trans, cond_torsions, seqres, tables, use_graph)

    def _rollout(self, key, fn, call, pad, zs, mask, cond_rots, cond_trans, cond_torsions, seqres, tables, use_graph):
        """The body of rollout_euler / rollout_rk on the staging set `key`: the library function `fn`, and `call(B, T, L)` ->
        (fn's scalar arguments ahead of the block count, the workspace).  `pad`: the staged noise keeps every block on 16 bytes
        -- a block stride rounded up to 4 floats, handed to `fn` after zs -- where B*T*L*D is no multiple of 4; else the blocks
        lie contiguous and `fn` takes no stride."""
        if self._pre_run is not None:
            self._pre_run()
        if zs.dim() != 5 or zs.shape[-1] != self.cfg.latent_dim:
            raise L.MdgenError(f"zs must be (R,B,T,L,{self.cfg.latent_dim}), got {tuple(zs.shape)}")
        R, B, T, L_, D = zs.shape
        require_cuda(zs, mask, cond_rots, cond_trans, cond_torsions, seqres)
        scalars, ws = call(B, T, L_)
        blk = B * T * L_ * D
        stride = (blk + 3) // 4 * 4 if pad else blk
        f32, i64 = torch.float32, torch.int64
        spec = dict(zs=((R, stride) if pad else (R, B, T, L_, D), f32), mask=((B, T, L_), f32), rots=((B, L_, 3, 3), f32),
                    trans=((B, L_, 3), f32), tors=((B, L_, 7, 2), f32), seqres=((B, L_), i64), x_cond=((B, T, L_, D), f32),
                    x_cond_mask=((B, T, L_), i64), atom14=((B, R * T, L_, 14, 3), f32))
        stg = self._staged((key, R, B, T, L_), spec, dict(mask=mask, rots=cond_rots, trans=cond_trans, tors=cond_torsions, seqres=seqres))
        staged_zs = stg["zs"].view(R, stride)[:, :blk]
        staged_zs.copy_(zs.reshape(R, blk))
        tb = L.ResidueTables.from_dict(tables)
        sh = L.Shape(B, T, L_)
        with self._call_stream(use_graph) as stream:
            check(fn(self._ctx, C.byref(sh), *scalars, R, ptr(stg["zs"]), *([stride] if pad else []), ptr(stg["mask"]),
                     ptr(stg["rots"]), ptr(stg["trans"]), ptr(stg["tors"]), ptr(stg["seqres"]), ptr(stg["x_cond"]),
                     ptr(stg["x_cond_mask"]), C.byref(tb), ptr(stg["atom14"]), ptr(ws), ws.numel(), int(use_graph), stream))
        nxt = {"rots": stg["rots"].clone(), "trans": stg["trans"].clone(), "torsions": stg["tors"].clone()}
        return stg["atom14"].clone(), staged_zs.reshape(R, B, T, L_, D).clone(), nxt

    def _rk_call(self, method, num_steps, B, T, L_):
        """((method code, S), workspace) of a fixed-grid Runge-Kutta call of this shape: one workspace for sample_rk and the drivers."""
        code = L.RK_METHODS.get(method)
        if code is None:
            raise L.MdgenError(f"method must be one of {sorted(L.RK_METHODS)}, got {method!r}")
        S = int(num_steps)
        if S < 1:
            raise L.MdgenError(f"num_steps must be >= 1, got {num_steps}")
        sh = L.Shape(B, T, L_)
        nbytes = C.c_size_t()
        check(lib.mdgen_rk_workspace_bytes(self._ctx, C.byref(sh), code, S, C.byref(nbytes)))
        return (code, S), self._sized_workspace(("rk", B, T, L_), nbytes.value)

    def rollout_rk(self, zs, method: str, num_steps: int, mask, cond_rots, cond_trans, cond_torsions, seqres, tables,
                   use_graph: bool = True):
        """`mdgen_rollout_rk`: `rollout_euler` with `method` in ("midpoint", "heun3", "rk4") solving every block in `num_steps`
        steps (as `sample_rk`), still one call and one hipGraph.  Arguments and return values as `rollout_euler`.  The staged
        noise is padded (`_rollout`); the padding never leaves this class."""
        return self._rollout("rollout_rk", lib.mdgen_rollout_rk, lambda *shape: self._rk_call(method, num_steps, *shape), True,
                             zs, mask, cond_rots, cond_trans, cond_torsions, seqres, tables, use_graph)

    def rollout_sde(self, zs, opts, rng, mask, cond_rots, cond_trans, cond_torsions, seqres, tables, use_graph: bool = True):
        """`mdgen_rollout_sde`: `rollout_rk` with the SDE solve of `sample_sde(..., rng=rng)` per block -- block k draws its noise
        with the counter word block_base + k -- still one call and one hipGraph, and no noise is staged.  Arguments and return
        values as `rollout_euler`."""
        self._check_rng(rng)
        return self._rollout("rollout_rk", lib.mdgen_rollout_sde,
                             lambda *shape: ((C.byref(opts), ptr(rng)), self._sde_workspace(opts, *shape)), True,
                             zs, mask, cond_rots, cond_trans, cond_torsions, seqres, tables, use_graph)

    # ---- trajectory upsampling ---------------------------------------------------------------
    def _upsample(self, fn, call, zs, cond_interval, mask, key_rots, key_trans, key_torsions, seqres, tables, use_graph):
        """The body of upsample_euler / upsample_rk: the checks of an upsampling call, its staging set (one per shape and
        interval, shared by the solvers) and the library function `fn`; `call(B, T, L)` -> (fn's scalar arguments ahead of the
        interval, the workspace)."""
        if self._pre_run is not None:
            self._pre_run()
        if self.cfg.tps_condition:
            raise L.MdgenError("upsample_euler is defined for forward-simulation models (sim_condition)")
        if zs.dim() != 4 or zs.shape[-1] != self.cfg.latent_dim:
            raise L.MdgenError(f"zs must be (B,T,L,{self.cfg.latent_dim}), got {tuple(zs.shape)}")
        B, T, L_, D = zs.shape
        c = int(cond_interval)
        if c < 1:
            raise L.MdgenError(f"cond_interval must be >= 1, got {cond_interval}")
        K = -(-T // c)
        if tuple(key_rots.shape) != (B, K, L_, 3, 3) or tuple(key_trans.shape) != (B, K, L_, 3) or \
                tuple(key_torsions.shape) != (B, K, L_, 7, 2):
            raise L.MdgenError(f"key frames must be (B,K,L,...) with K = ceil(T / cond_interval) = {K}: got rots "
                               f"{tuple(key_rots.shape)}, trans {tuple(key_trans.shape)}, torsions {tuple(key_torsions.shape)}")
        if tuple(mask.shape) != (B, T, L_):
            raise L.MdgenError(f"mask must be (B,T,L)={B, T, L_}, got {tuple(mask.shape)}")
        require_cuda(zs, mask, key_rots, key_trans, key_torsions, seqres)
        f32, i64 = torch.float32, torch.int64
        spec = dict(zs=((B, T, L_, D), f32), mask=((B, T, L_), f32), rots=((B, K, L_, 3, 3), f32), trans=((B, K, L_, 3), f32),
                    tors=((B, K, L_, 7, 2), f32), seqres=((B, L_), i64), x_cond=((B, T, L_, D), f32), x_cond_mask=((B, T, L_), i64),
                    sr=((B, L_, 3, 3), f32), st=((B, L_, 3), f32), atom14=((B, T, L_, 14, 3), f32))
        stg = self._staged(("upsample", B, T, L_, c), spec,
                           dict(zs=zs, mask=mask, rots=key_rots, trans=key_trans, tors=key_torsions, seqres=seqres))
        scalars, ws = call(B, T, L_)
        tb = L.ResidueTables.from_dict(tables)
        sh = L.Shape(B, T, L_)
        with self._call_stream(use_graph) as stream:
            check(fn(self._ctx, C.byref(sh), *scalars, c, ptr(stg["zs"]), ptr(stg["mask"]), ptr(stg["rots"]), ptr(stg["trans"]),
                     ptr(stg["tors"]), ptr(stg["seqres"]), ptr(stg["x_cond"]), ptr(stg["x_cond_mask"]), ptr(stg["sr"]),
                     ptr(stg["st"]), C.byref(tb), ptr(stg["atom14"]), ptr(ws), ws.numel(), int(use_graph), stream))
        return stg["atom14"].clone(), stg["zs"].clone()

    def upsample_euler(self, zs, num_steps: int, cond_interval: int, mask, key_rots, key_trans, key_torsions, seqres, tables,
                       use_graph: bool = True):
        """`mdgen_upsample_euler`: key-frame conditioning -> S Euler steps -> atom14 in one call (one hipGraph).  zs (B,T,L,D)
        noise, one window per batch element; mask (B,T,L); key_* the K = ceil(T / cond_interval) key frames of every window,
        (B,K,L,...); seqres (B,L) int64; tables: dict of residue tables on the device (geometry.residue_tables).
        Returns (atom14 (B,T,L,14,3), samples (B,T,L,D))."""
        S = int(num_steps)
        return self._upsample(lib.mdgen_upsample_euler, lambda *shape: ((S,), self._workspace(*shape, S, True)),
                              zs, cond_interval, mask, key_rots, key_trans, key_torsions, seqres, tables, use_graph)

    def upsample_rk(self, zs, method: str, num_steps: int, cond_interval: int, mask, key_rots, key_trans, key_torsions, seqres,
                    tables, use_graph: bool = True):
        """`mdgen_upsample_rk`: `upsample_euler` with `method` in ("midpoint", "heun3", "rk4") solving the windows in `num_steps`
        steps (as `sample_rk`): key-frame conditioning -> solve -> atom14 in one call (one hipGraph).  Arguments and return
        values as `upsample_euler`."""
        return self._upsample(lib.mdgen_upsample_rk, lambda *shape: self._rk_call(method, num_steps, *shape),
                              zs, cond_interval, mask, key_rots, key_trans, key_torsions, seqres, tables, use_graph)

    def upsample_sde(self, zs, opts, rng, cond_interval: int, mask, key_rots, key_trans, key_torsions, seqres, tables,
                     use_graph: bool = True):
        """`mdgen_upsample_sde`: `upsample_rk` with the SDE solve of `sample_sde(..., rng=rng)`: key-frame conditioning -> solve ->
        atom14 in one call (one hipGraph), no noise staged.  Arguments and return values as `upsample_euler`."""
        self._check_rng(rng)
        return self._upsample(lib.mdgen_upsample_sde, lambda *shape: ((C.byref(opts), ptr(rng)), self._sde_workspace(opts, *shape)),
                              zs, cond_interval, mask, key_rots, key_trans, key_torsions, seqres, tables, use_graph)
