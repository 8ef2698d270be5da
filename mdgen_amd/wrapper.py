"""`NewMDGenWrapper` -- drop-in for the inference surface of `mdgen.wrapper.NewMDGenWrapper`
(wrapper.py:175-221 `__init__`, :283-365 `prep_batch`, :405-484 `inference`) plus
`load_from_checkpoint` for Lightning-format checkpoints (SURVEY.md section 5 "Checkpoint / resume"),
without Lightning.  The training step (`general_step` forward half here; backward, optimiser, EMA, DDP in
`mdgen_amd/train.py`) runs in the same library; Lightning's logging hooks are out of scope."""
from __future__ import annotations

import argparse
import ctypes as C
from functools import partial

import torch

from . import _lib as L
from ._lib import lib, launch, ptr, require_cuda
from .config import ModelConfig
from .geometry import prep_keyframes, samples_to_atom14
from .model import LatentMDGenModel
from .rigid_utils import Rigid, Rotation
from .solver import RK_DEFAULT_STEPS, SDE_DEFAULT_STEPS, SDE_DEFAULTS, resolve_solver, sde_opts  # noqa: F401 (the defaults are named from here)
from .transport import Sampler, create_transport

_BACKFILL = ["inpainting", "no_torsion", "hyena", "no_aa_emb", "supervise_all_torsions", "supervise_no_torsions",
             "design_key_frames", "no_design_torsion", "cond_interval", "mpnn", "dynamic_mpnn", "no_offsets",
             "no_frames", "design", "tps_condition", "sim_condition", "abs_pos_emb", "prepend_ipa", "oracle"]
_UNSUPPORTED = ["inpainting", "hyena", "no_aa_emb", "design_key_frames", "mpnn", "dynamic_mpnn", "no_offsets",
                "no_frames", "design", "no_torsion", "no_design_torsion", "interleave_ipa",
                "abs_time_emb", "oracle", "no_rope"]


def default_args(cfg: ModelConfig) -> argparse.Namespace:
    a = argparse.Namespace(**cfg.to_dict())
    a.path_type, a.prediction, a.sampling_method = "GVP", "velocity", "euler"
    return a


class NewMDGenWrapper:
    def __init__(self, args, device="cuda", precision="bf16"):
        if isinstance(args, ModelConfig):
            args = default_args(args)
        for k in _BACKFILL:                       # wrapper.py:178-194: newer flags default to False
            if not hasattr(args, k):
                setattr(args, k, False)
        bad = [k for k in _UNSUPPORTED if getattr(args, k, False)]
        if bad:
            raise L.MdgenError(f"flags outside the accelerated sampler path: {bad}")
        if not getattr(args, "prepend_ipa", False):
            raise L.MdgenError("the accelerated path implements the prepend_ipa models (README.md:48,60)")
        # latent_model.py:183-207 tests sim_condition first and tps_condition second, and only these two branches
        # set up the IPA inputs; wrapper.py:339-342 marks the conditioning frames for exactly one of them.  A
        # checkpoint with both flags or neither would silently run something else here: reject it.
        if bool(args.sim_condition) == bool(args.tps_condition):
            raise L.MdgenError("exactly one of sim_condition / tps_condition must be set "
                               f"(got sim_condition={args.sim_condition}, tps_condition={args.tps_condition})")
        self.args = args
        self.cfg = ModelConfig.from_args(args)
        self.latent_dim = self.cfg.latent_dim
        self.device = torch.device(device)
        self.model = LatentMDGenModel(self.cfg, self.device, precision=precision)
        self.transport = create_transport(args, getattr(args, "path_type", "GVP"), getattr(args, "prediction", "velocity"))
        self.transport_sampler = Sampler(self.transport)

    # Lightning surface used by the drivers (sim_inference.py:129-130)
    @classmethod
    def load_from_checkpoint(cls, path, device="cuda", precision="bf16"):
        ckpt = torch.load(path, map_location="cpu", weights_only=False)
        args = ckpt["hyper_parameters"]["args"]
        w = cls(args, device=device, precision=precision)
        sd = {k[len("model."):]: v for k, v in ckpt["state_dict"].items() if k.startswith("model.")}
        w.load_model_state_dict(sd)
        w.ema_state = ckpt.get("ema")            # wrapper.py:120-124 `on_load_checkpoint`
        return w

    # wrapper.py:64-76: validation runs on the EMA weights and restores the raw ones afterwards
    def load_ema_weights(self, ema_params=None):
        """Swap the EMA parameters in (`ema_params`: a full state dict; default: the checkpoint's `ema['params']`)."""
        if ema_params is None:
            if not getattr(self, "ema_state", None):
                raise L.MdgenError("no EMA state: the checkpoint has no 'ema' entry (trained without --ema)")
            ema_params = self.ema_state["params"]
        if not hasattr(self, "model_state_dict"):
            raise L.MdgenError("load_ema_weights needs the raw weights to restore later: use load_model_state_dict()")
        # the weights to restore are the CURRENT ones: a Trainer attached to this wrapper has moved on from what was loaded
        tr = getattr(self, "trainer", None)
        tr = tr() if tr is not None else None          # (`Trainer` leaves a weak reference here)
        self.cached_weights = ({k: v.detach().clone() for k, v in tr.tm.state_dict().items()} if tr is not None
                               else self.model_state_dict)
        self.model.load_state_dict({k: v for k, v in ema_params.items()})
        return self

    def restore_cached_weights(self):
        if getattr(self, "cached_weights", None) is not None:
            self.model.load_state_dict(self.cached_weights)
            self.cached_weights = None
        return self

    def load_model_state_dict(self, sd):
        """Hand the `model.*` tensors to the library and remember them (the training step starts from them)."""
        self.model.load_state_dict(sd)
        self.model_state_dict = {k: v.detach().clone() for k, v in sd.items()}
        return self

    def eval(self):
        return self

    def to(self, device):
        self.model.to(device)
        return self

    # ---------------------------------------------------------------------------------------------
    def prep_batch(self, batch):
        """wrapper.py:283-365 (sim_condition / tps_condition paths)."""
        trans = batch["trans"].to(torch.float32).contiguous()
        rots = batch["rots"].to(torch.float32).contiguous()
        tors = batch["torsions"].to(torch.float32).contiguous()
        require_cuda(trans, rots, tors)
        B, T, L_ = trans.shape[:3]
        tps = bool(self.args.tps_condition)
        D = self.latent_dim
        dev = trans.device
        latents = torch.empty(B, T, L_, D, device=dev)
        x_cond = torch.empty(B, T, L_, D, device=dev)
        cond_mask = torch.empty(B, T, L_, dtype=torch.int64, device=dev)
        sh = L.Shape(B, T, L_)
        launch(lib.mdgen_prep_latents, trans, C.byref(sh), int(tps), int(getattr(self.args, "cond_interval", 0) or 0),
               ptr(rots), ptr(trans), ptr(tors), ptr(latents),
               ptr(x_cond), ptr(cond_mask))
        rigids = Rigid(Rotation(rot_mats=rots), trans)
        mask = batch["mask"].to(torch.float32)
        frame_lm = mask.unsqueeze(-1).expand(-1, -1, 7)
        if tps:
            frame_lm = torch.cat([frame_lm, frame_lm], -1)
        tors_lm = batch["torsion_mask"].unsqueeze(-1).expand(-1, -1, -1, 2).reshape(B, L_, 14)
        if getattr(self.args, "supervise_all_torsions", False):
            tors_lm = torch.ones_like(tors_lm)
        elif getattr(self.args, "supervise_no_torsions", False):
            tors_lm = torch.zeros_like(tors_lm)
        loss_mask = torch.cat([frame_lm, tors_lm.to(frame_lm.dtype)], -1).unsqueeze(1).expand(-1, T, -1, -1)
        return {
            "rigids": rigids,
            "latents": latents,
            "loss_mask": loss_mask,
            "model_kwargs": {
                "start_frames": rigids[:, 0],
                "end_frames": rigids[:, -1],
                "mask": mask.unsqueeze(1).expand(-1, T, -1),
                "aatype": batch["seqres"],
                "x_cond": x_cond,
                "x_cond_mask": cond_mask,
            },
        }

    def general_step(self, batch, stage="val", t=None, x0=None):
        """The forward half of wrapper.py:367-384 `general_step`: `prep_batch` -> `transport.training_losses`
        (flow-matching target, model forward, masked MSE).  Returns the loss per sample (B,) and the term dict.
        The backward pass + optimiser step of the same quantities is `mdgen_amd.train.Trainer.training_step`; `stage` is
        informational; `t` and `x0` may be fixed for reproducibility (the reference draws them inside the transport)."""
        prep = self.prep_batch(batch)
        out = self.transport.training_losses(model=self.model.forward, x1=prep["latents"], aatype1=None,
                                             mask=prep["loss_mask"], model_kwargs=prep["model_kwargs"], t=t, x0=x0)
        return out["loss"], out

    def _solver(self, sampling_method, num_steps, atol, rtol, sde, noise=None, rng_seed=None, rng_sample_base=0, rng_block_base=0):
        """The call's `solver.SolverChoice` (every refusal about solver arguments is `resolve_solver`'s)."""
        return resolve_solver(getattr(self.args, "sampling_method", "euler"), sampling_method, num_steps, atol, rtol, sde,
                              getattr(self.args, "path_type", "GVP"), noise, rng_seed, rng_sample_base, rng_block_base)

    def _rng(self, choice, sample_base, block_base):
        """The wrapper's four device words {seed, sample_base, block_base, 0} (`mdgen_sample_sde_rng`), written on the current
        stream for this call; None without `rng_seed`.  One buffer for every call: a captured graph reads it at replay."""
        if choice.rng_seed is None:
            return None
        if getattr(self, "_rng_words", None) is None:
            self._rng_words = torch.zeros(4, dtype=torch.int64, device=self.device)
        self._rng_words.copy_(L.rng_words(choice.rng_seed, sample_base, block_base))
        return self._rng_words

    def _sde_opts(self, sampling_method, num_steps, sde):
        return sde_opts(sampling_method, num_steps, sde, self.args.path_type)

    def inference(self, batch, zs=None, num_steps=None, use_graph=True, rel_quats=None, sampling_method=None, atol=1e-6,
                  rtol=1e-3, sde=None, noise=None, rng_seed=None, rng_sample_base=0, rng_block_base=0):
        """wrapper.py:405-484.  Extra keywords (defaults reproduce the reference): `zs` explicit noise
        (reference: device randn, wrapper.py:439), `num_steps` Euler steps S (reference: 50 grid points = 49
        steps, wrapper.py:441-442 / transport.py:412), `rel_quats` (two-sided models): the relative-frame 7-vectors
        (2,B,L,7) as the caller's reference computes them (`LatentMDGenModel._rel7`; default: w >= 0 convention).
        `sampling_method="dopri5"`: the reference's adaptive solver (torchdiffeq dopri5 with `atol` / `rtol`,
        `LatentMDGenModel.sample_dopri5`; one step size for the whole batch); its counts are kept in `last_stats`.
        `sampling_method="midpoint" | "heun3" | "rk4"`: torchdiffeq's fixed-grid solvers with `num_steps` steps S on
        linspace(0, 1, S + 1) (`LatentMDGenModel.sample_rk`, one hipGraph; default 24 / 16 / 12 steps = 48 network evaluations);
        a sample's solution does not depend on its batch mates.
        `sampling_method="sde" | "sde_heun"`: the reference's `Sampler.sample_sde` with Euler-Maruyama / Heun steps
        (`LatentMDGenModel.sample_sde`, one hipGraph): `num_steps` stochastic steps S (default 49) on S + 1 grid points, then the
        last step; `sde`: a dict over SDE_DEFAULTS (diffusion_form "sigma", diffusion_norm 1, last_step "Mean", last_step_size
        0.04, sample_eps 0); `noise`: optional (S, B, T, L, D) standard normals, default a device randn drawn after `zs`.
        `rng_seed` (sde / sde_heun, never with `noise`): the kernels generate the noise from this 64-bit seed with Philox4x32-10
        at each element's coordinates (`mdgen_sample_sde_rng`, include/mdgen_amd.h) -- no (S, B, T, L, D) buffer exists, and the
        noise of sample b is that of sample index `rng_sample_base` + b, of block index `rng_block_base`: whichever batch a
        sample travels in, the same indices give it the same noise.
        The solver arguments are judged by `solver.resolve_solver`, before the batch is touched."""
        choice = self._solver(sampling_method, num_steps, atol, rtol, sde, noise, rng_seed, rng_sample_base, rng_block_base)
        return self._inference(batch, choice, zs=zs, use_graph=use_graph, rel_quats=rel_quats, noise=noise,
                               rng=self._rng(choice, rng_sample_base, rng_block_base))

    def _inference(self, batch, choice, zs=None, use_graph=True, rel_quats=None, noise=None, rng=None):
        """`inference()` with its solver resolved."""
        prep = self.prep_batch(batch)
        rigids = prep["rigids"]
        B, T, L_ = rigids.shape
        dev = prep["latents"].device
        if zs is None:
            zs = torch.randn(B, T, L_, self.latent_dim, device=dev)
        kw = dict(prep["model_kwargs"])
        kw["mask"] = kw["mask"].contiguous()
        if not self.args.tps_condition:
            kw["end_frames"] = None
        if rel_quats is not None:
            kw["rel_quats"] = rel_quats
        if choice.kind == "dopri5":
            samples, self.last_stats = self.model.sample_dopri5(zs, atol=choice.atol, rtol=choice.rtol, **kw)
        elif choice.kind == "sde":
            samples = self.model.sample_sde(zs, choice.sde_opts, noise=noise, use_graph=use_graph, rng=rng, **kw)
        else:   # "euler" | "rk": the transport's fixed-grid samplers
            sample_fn = self.transport_sampler.sample_ode(sampling_method=choice.method, num_steps=choice.steps + 1)
            samples = sample_fn(zs, partial(self.model.forward_inference, **kw), use_graph=use_graph)[-1]
        r0 = rigids[:, 0]
        atom14 = samples_to_atom14(samples, r0.get_rots().get_rot_mats(), r0.get_trans(), batch["seqres"],
                                   bool(self.args.tps_condition))
        aa_out = batch["seqres"][:, None].expand(B, T, L_)
        self.last_samples = samples
        return atom14, aa_out

    def upsample(self, batch, num_frames=None, zs=None, num_steps=None, use_graph=True, sampling_method=None, atol=1e-6,
                 rtol=1e-3, sde=None, rng_seed=None, rng_sample_base=0, rng_block_base=0):
        """Trajectory upsampling: sample the frames between key frames stored every `args.cond_interval` frames
        (upsampling_inference.py:47-82 around `inference`, wrapper.py:405-484).  `batch` holds KEY FRAMES only, one window per
        batch element: torsions (B,K,L,7,2), trans (B,K,L,3), rots (B,K,L,3,3), seqres (B,L), mask (B,L), with
        K = ceil(T / cond_interval) and T = `num_frames` (default `args.num_frames`); key frame k is frame k * cond_interval of
        its window.  Euler: one library call (`mdgen_upsample_euler`, one hipGraph); "midpoint" | "heun3" | "rk4": likewise
        (`mdgen_upsample_rk`; `num_steps` steps, default 24 / 16 / 12).  `sampling_method="dopri5"`:
        `mdgen_prep_keyframes` -> `sample_dopri5` -> `samples_to_atom14`, counts in `last_stats`; "sde" | "sde_heun" (with `sde`,
        as `inference()`): the same three calls around `sample_sde` -- or, with `rng_seed` (`rng_sample_base`, `rng_block_base`: as
        `inference()`), one library call and one hipGraph like the other fixed-grid solvers (`mdgen_upsample_sde`), the noise
        generated in the kernels.  The solver rules are `inference()`'s.  Returns (atom14 (B,T,L,14,3), aa_out (B,T,L)); the latent samples are kept in `last_samples`."""
        from .geometry import residue_tables
        c = getattr(self.args, "cond_interval", None)
        if not c:
            raise L.MdgenError("upsample() needs a model trained with --cond_interval (args.cond_interval is not set)")
        if self.args.tps_condition:
            raise L.MdgenError("upsample() is defined for forward-simulation models (sim_condition), not two-sided ones")
        c = int(c)
        T = int(self.args.num_frames if num_frames is None else num_frames)
        if c < 1 or T < 1:
            raise L.MdgenError(f"num_frames and cond_interval must be >= 1, got {T}, {c}")
        choice = self._solver(sampling_method, num_steps, atol, rtol, sde, None, rng_seed, rng_sample_base, rng_block_base)
        tors = batch["torsions"].to(torch.float32)
        trans = batch["trans"].to(torch.float32)
        rots = batch["rots"].to(torch.float32)
        require_cuda(tors, trans, rots)
        if trans.dim() != 4:
            raise L.MdgenError(f"key-frame batch: trans must be (B,K,L,3), got {tuple(trans.shape)}")
        B, K, L_ = trans.shape[:3]
        if K != -(-T // c):
            raise L.MdgenError(f"{K} key frames per window, but num_frames={T} with cond_interval={c} needs "
                               f"ceil({T} / {c}) = {-(-T // c)}")
        dev = trans.device
        if zs is None:
            zs = torch.randn(B, T, L_, self.latent_dim, device=dev)
        mask = batch["mask"].to(torch.float32).unsqueeze(1).expand(-1, T, -1)
        if choice.kind == "sde" and choice.rng_seed is not None:
            atom14, samples = self.model.upsample_sde(zs, choice.sde_opts, self._rng(choice, rng_sample_base, rng_block_base), c, mask,
                                                      rots, trans, tors, batch["seqres"], residue_tables(dev), use_graph=use_graph)
        elif choice.kind in ("dopri5", "sde"):
            prep = prep_keyframes(rots, trans, tors, T, c)
            kw = dict(mask=mask.contiguous(), start_frames=(prep["start_rot"], prep["start_trans"]), x_cond=prep["x_cond"],
                      x_cond_mask=prep["x_cond_mask"], aatype=batch["seqres"])
            if choice.kind == "sde":
                samples = self.model.sample_sde(zs, choice.sde_opts, use_graph=use_graph, **kw)
            else:
                samples, self.last_stats = self.model.sample_dopri5(zs, atol=choice.atol, rtol=choice.rtol, **kw)
            atom14 = samples_to_atom14(samples, prep["start_rot"], prep["start_trans"], batch["seqres"], False)
        elif choice.kind == "rk":
            atom14, samples = self.model.upsample_rk(zs, choice.method, choice.steps, c, mask, rots, trans, tors, batch["seqres"],
                                                     residue_tables(dev), use_graph=use_graph)
        else:
            atom14, samples = self.model.upsample_euler(zs, choice.steps, c, mask, rots, trans, tors, batch["seqres"],
                                                        residue_tables(dev), use_graph=use_graph)
        self.last_samples = samples
        return atom14, batch["seqres"][:, None].expand(B, T, L_)

    def _rollout_host_loop(self, batch, T, zs, choice, use_graph):
        """The blocks of `rollout()` as a host loop of `inference()` with the resolved `choice` -- prep_latents -> the solver -> samples_to_atom14 --
        and `atom14_to_cond`, all on the device: the adaptive solver (dopri5 reads its error ratio back once per attempted step,
        so it cannot be captured) and the SDE samplers with staged noise (their fused driver generates its noise: `rng_seed`).  -> (atom14, samples (R,B,T,L,D), next conditioning
        frame, per-block stats)."""
        from .geometry import atom14_to_cond
        out, samples, stats = [], [], []
        for z in zs:
            ex = dict(batch)
            ex["torsions"] = batch["torsions"].expand(-1, T, -1, -1, -1)
            ex["trans"] = batch["trans"].expand(-1, T, -1, -1)
            ex["rots"] = batch["rots"].expand(-1, T, -1, -1, -1)
            atom14, _ = self._inference(ex, choice, zs=z, use_graph=use_graph)
            nxt = atom14_to_cond(atom14[:, -1], batch["seqres"])
            batch = dict(batch)
            batch["trans"], batch["rots"], batch["torsions"] = nxt["trans"][:, None], nxt["rots"][:, None], nxt["torsions"][:, None]
            out.append(atom14)
            samples.append(self.last_samples)
            stats.append(getattr(self, "last_stats", None))
        return torch.cat(out, 1), torch.stack(samples), nxt, stats

    def rollout(self, batch, num_frames: int, num_rollouts: int, num_steps=None, zs=None, use_graph=True,
                return_next: bool = False, sampling_method=None, atol=1e-6, rtol=1e-3, sde=None, rng_seed=None, rng_sample_base=0,
                rng_block_base=0):
        """`num_rollouts` chained blocks of `num_frames` frames from the B = 1-frame conditioning batch of
        `sim_inference.get_batch` (torsions (B,1,L,7,2), trans (B,1,L,3), rots (B,1,L,3,3), seqres, mask (B,L)):
        the loop of sim_inference.py:100-113 (`rollout` :61-98 per block) as ONE library call, captured as one hipGraph:
        `mdgen_rollout_euler` (`sampling_method` None or "euler"; None refuses a non-Euler checkpoint unless `num_steps` is
        given) or `mdgen_rollout_rk` ("midpoint" | "heun3" | "rk4", `num_steps` steps per block, default 24 / 16 / 12).
        "dopri5" (with `atol` / `rtol`, no `num_steps`) is a host loop over the blocks with the same device glue -- the solver
        reads back once per attempted step -- and leaves a list of per-block counts in `last_stats`; "sde" | "sde_heun" (with `sde`,
        as `inference()`) run as the same host loop, one `sample_sde` graph per block -- or, with `rng_seed`, as ONE library call
        and one hipGraph (`mdgen_rollout_sde`): the kernels generate the noise, block k's with the block index `rng_block_base` + k
        and sample b's with the sample index `rng_sample_base` + b (as `inference()`).  `zs`: optional noise
        (num_rollouts, B, T, L, D); without it a block's noise is a fresh device randn (wrapper.py:439), drawn block by block
        when a method is named.  Returns atom14 (B, num_rollouts*T, L, 14, 3) [, the batch that would condition the next
        block]; the latent samples (num_rollouts, B, T, L, D) are kept in `last_samples`."""
        from .geometry import residue_tables
        if self.args.tps_condition or getattr(self.args, "cond_interval", None):
            raise L.MdgenError("rollout() is the forward-simulation driver (sim_condition models without cond_interval)")
        choice = self._solver(sampling_method, num_steps, atol, rtol, sde, None, rng_seed, rng_sample_base, rng_block_base)
        tors = batch["torsions"][:, 0].to(torch.float32)
        trans = batch["trans"][:, 0].to(torch.float32)
        rots = batch["rots"][:, 0].to(torch.float32)
        require_cuda(tors, trans, rots)
        B, L_ = trans.shape[:2]
        T, R = int(num_frames), int(num_rollouts)
        dev = trans.device
        if zs is None and choice.kind == "euler":
            zs = torch.randn(R, B, T, L_, self.latent_dim, device=dev)
        elif zs is None:   # one draw per block, in block order: what the per-block loop of inference() calls draws
            zs = torch.stack([torch.randn(B, T, L_, self.latent_dim, device=dev) for _ in range(R)])
        mask = batch["mask"].to(torch.float32).unsqueeze(1).expand(-1, T, -1)
        if choice.kind == "sde" and choice.rng_seed is not None:
            atom14, samples, nxt = self.model.rollout_sde(zs, choice.sde_opts, self._rng(choice, rng_sample_base, rng_block_base), mask,
                                                          rots, trans, tors, batch["seqres"], residue_tables(dev), use_graph=use_graph)
        elif choice.kind in ("dopri5", "sde"):
            atom14, samples, nxt, stats = self._rollout_host_loop(batch, T, zs, choice, use_graph)
            if choice.kind == "dopri5":
                self.last_stats = stats
        elif choice.kind == "rk":
            atom14, samples, nxt = self.model.rollout_rk(zs, choice.method, choice.steps, mask, rots, trans, tors, batch["seqres"],
                                                         residue_tables(dev), use_graph=use_graph)
        else:
            atom14, samples, nxt = self.model.rollout_euler(zs, choice.steps, mask, rots, trans, tors, batch["seqres"],
                                                            residue_tables(dev), use_graph=use_graph)
        self.last_samples = samples
        if not return_next:
            return atom14
        new = dict(batch)
        new["trans"], new["rots"], new["torsions"] = nxt["trans"][:, None], nxt["rots"][:, None], nxt["torsions"][:, None]
        return atom14, new
