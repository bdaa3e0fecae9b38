"""One federated round on the engine (the body of ExperimentRunner.run_simulation,
experiments/run_experiments.py:188-259, minus evaluation and checkpointing).

  for each client: fresh model <- global; local SGD                (:193-240)
  malicious clients submit a poisoned update                       (malicious_client.py:103-115)
  aggregated = defense.aggregate(client_updates, num_examples)     (:243-254)
  global params <- aggregated                                      (:257-259)

The K clients are sharded over the GPUs (flr.dist); each GPU trains its rows
of the client matrix together.  The exchange is then either
* "alltoall" (default for FedAvg / Krum / trimmed mean / median): one
  all-to-all hands every GPU all K clients' values of its coordinate range
  (flr.shard), each GPU aggregates its range, and one all-gather of the
  P-vector slices rebuilds the global model; or
* "allgather": one all-gather assembles the whole K×P matrix on every GPU and
  the aggregation runs replicated (defenses that need whole rows).
Both give the bit-identical global model at every GPU count.
"""
from __future__ import annotations

import logging
import os
from dataclasses import dataclass, field
from typing import Dict, Optional

import torch

from . import _capi
from . import dist as fdist
from . import ops
from .attacks import (PERTURBATIONS, Backdoor, alie_z, fang_krum_config, fang_trim_config, poison_batches_,
                      replace_rows_, replacement_config)
from .defenses import get_defense
from .defenses.krum import DeadTaps
from .matrix import ClientMatrix
from .shard import PW_SLICES, Comm, CoordExchange, aligned_bounds
from .models.multimodal import ModelSpec, model_class, param_layout
from .train import ClientBatchTrainer, TrainConfig, make_dropout_masks, synthetic_batches


ATTACKS = ("sign_flip", "backdoor", "none", "alie", "ipm", "min_max", "min_sum", "model_replacement", "fang_krum",
           "fang_trim")


@dataclass
class RoundConfig:
    num_clients: int = 128
    batch: int = 32                      # run_experiments.py:40
    defense: str = "krum"
    defense_cfg: Dict = field(default_factory=dict)
    # "sign_flip" (model_poisoning.py:274-276) | "backdoor" | "none" | "alie" | "ipm" (the colluding attacks of
    # flr.attacks: one flr_collude_rows pass between the exchange and the defense) | "min_max" | "min_sum" (one
    # flr_minmax_rows call in the same slot; whole rows: the all-gather exchange unless world == 1) |
    # "model_replacement" (the backdoor's data, then the attackers' rows boosted about the global model in that slot) |
    # "fang_krum" (Fang et al.'s Krum attack, one flr_fang_krum_rows call in that slot; whole rows, as min_max) |
    # "fang_trim" (their trimmed-mean attack, one coordinate-wise flr_fang_trim_rows pass; runs on an all-to-all slice)
    attack: str = "sign_flip"
    num_attackers: int = 25              # f = int(0.2 K), clients 0..f-1 (experiment_matrix.py:67-68)
    seed: int = 42                       # run_experiments.py:43
    exchange: str = "auto"               # "alltoall" | "allgather" | "auto" (alltoall when the defense shards)
    graph: bool = True                   # replay the training phase as one captured HIP graph (FLR_GRAPH=0: eager)
    fallback_fedavg: bool = False        # defense raises -> FedAvg of the round (robust_server.py:120-122)
    # with fallback_fedavg: also fall back on library / device errors (FlrError,
    # out of memory), as the reference's `except Exception` does (the default:
    # ADVICE r5, parity with robust_server.py:120-122).  At world > 1 a device
    # error is never swallowed — one rank falling back while the others wait in
    # the defense's next collective would hang the round instead of failing it;
    # False keeps device errors loud at world 1 too
    fallback_device_errors: bool = True
    # "z" (alie; default alie_z(K, f)), "epsilon" (ipm; default 0.5), "perturb" (min_max / min_sum: "std" (default) |
    # "sign" | "unit", the direction of flr.attacks.min_max_); model_replacement: "boost" (default num_clients /
    # num_attackers), "stealth" ("none" (default) | "norm" | "distance"), "stat" (norm: "median" (default) | "max" |
    # "mean"), "rho" (default 1.0), the arguments of flr.attacks.model_replacement_; fang_krum: "threshold" (default
    # 1e-5); fang_trim: "b" (default 2.0), "seed" (default the round config's seed): flr.attacks.fang_krum_ / fang_trim_
    attack_cfg: Dict = field(default_factory=dict)


def initial_global(spec: ModelSpec, seed: int, device) -> torch.Tensor:
    """Global model init: the torch default init of the spec's model under seed."""
    torch.manual_seed(seed)
    m = model_class(spec)(spec)
    return torch.cat([p.detach().reshape(-1) for p in m.parameters()]).to(device)


class RoundEngine:
    def __init__(self, spec: ModelSpec, rcfg: RoundConfig, tcfg: TrainConfig = TrainConfig(), device="cuda",
                 rank: int = 0, world: int = 1):
        if rcfg.attack not in ATTACKS:  # a typo must not run as an unattacked round
            raise ValueError(f"unknown attack {rcfg.attack!r} (one of {', '.join(ATTACKS)})")
        # the colluding attacks: (mode, param) of the one flr_collude_rows call per round
        self._collude = None
        if rcfg.attack in ("alie", "ipm"):
            K, f = rcfg.num_clients, rcfg.num_attackers
            if not 1 <= f < K:
                raise ValueError(f"attack {rcfg.attack!r} needs 1 <= num_attackers < num_clients (got {f}, {K})")
            if rcfg.attack == "alie":
                z = rcfg.attack_cfg.get("z")
                self._collude = (ops.COLLUDE_ALIE, float(alie_z(K, f) if z is None else z))
            else:
                self._collude = (ops.COLLUDE_IPM, float(rcfg.attack_cfg.get("epsilon", 0.5)))
        # Min-Max / Min-Sum: (objective, perturbation) of the one flr_minmax_rows call per round;
        # attack_gamma: the last round's strength, a float64 device scalar (experiment logs)
        self._minmax = None
        self.attack_gamma: Optional[torch.Tensor] = None
        self.attack_status: Optional[torch.Tensor] = None  # model replacement: int32 [f] and int32 [1]
        self.attack_flags: Optional[torch.Tensor] = None   # (flr.attacks.model_replacement_)
        if rcfg.attack in ("min_max", "min_sum"):
            K, f = rcfg.num_clients, rcfg.num_attackers
            if not 1 <= f < K:
                raise ValueError(f"attack {rcfg.attack!r} needs 1 <= num_attackers < num_clients (got {f}, {K})")
            perturb = rcfg.attack_cfg.get("perturb", "std")
            if perturb not in PERTURBATIONS:
                raise ValueError(f"attack_cfg['perturb'] = {perturb!r}: one of {', '.join(PERTURBATIONS)}")
            if rcfg.exchange == "alltoall" and world > 1:  # "auto" takes the all-gather exchange below
                raise ValueError(f"attack {rcfg.attack!r} needs whole client rows (row distances, not a "
                                 "coordinate-wise statistic): use exchange='allgather' (a rank's all-to-all slice "
                                 "is the whole matrix only at world 1)")
            self._minmax = (ops.MINMAX_MAX if rcfg.attack == "min_max" else ops.MINMAX_SUM, PERTURBATIONS[perturb])
        # model replacement: (boost, mode, stat, rho) of the flr_replace_strength call per round; attack_gamma is
        # then the float64 [f] vector of the attackers' strengths
        self._replace = None
        self._replace_whole_rows = False
        if rcfg.attack == "model_replacement":
            unknown = set(rcfg.attack_cfg) - {"boost", "stealth", "stat", "rho"}
            if unknown:
                raise ValueError(f"attack_cfg keys {sorted(unknown)} are not model_replacement's "
                                 "(boost, stealth, stat, rho)")
            self._replace = replacement_config(rcfg.num_clients, rcfg.num_attackers, rcfg.attack_cfg.get("boost"),
                                               rcfg.attack_cfg.get("stealth", "none"),
                                               rcfg.attack_cfg.get("stat", "median"), rcfg.attack_cfg.get("rho", 1.0))
            self._replace_whole_rows = self._replace[1] != ops.REPLACE_NONE  # "auto" takes the all-gather below
            if self._replace_whole_rows and rcfg.exchange == "alltoall" and world > 1:
                raise ValueError(f"model_replacement with stealth {rcfg.attack_cfg['stealth']!r} needs whole client "
                                 "rows (row norms and distances, not a coordinate-wise statistic): use "
                                 "exchange='allgather' (a rank's all-to-all slice is the whole matrix only at "
                                 "world 1)")
        # Fang et al.'s attacks.  fang_krum: the threshold of the one flr_fang_krum_rows call per round; attack_gamma
        # is then lambda (a float64 device scalar) and attack_status its info, int32 [2]: status and halvings.
        # fang_trim: (b, seed) of the one flr_fang_trim_rows pass; its draws are keyed by the coordinate's index in
        # the order the matrix is held in (torch order here, col0 = the rank's first coordinate) and by the round
        self._fang_krum = self._fang_trim = None
        if rcfg.attack in ("fang_krum", "fang_trim"):
            keys = {"threshold"} if rcfg.attack == "fang_krum" else {"b", "seed"}
            unknown = set(rcfg.attack_cfg) - keys
            if unknown:
                raise ValueError(f"attack_cfg keys {sorted(unknown)} are not {rcfg.attack}'s "
                                 f"({', '.join(sorted(keys))})")
        if rcfg.attack == "fang_krum":
            self._fang_krum = fang_krum_config(rcfg.num_clients, rcfg.num_attackers,
                                               rcfg.attack_cfg.get("threshold", ops.FANG_THRESHOLD))
            if rcfg.exchange == "alltoall" and world > 1:  # "auto" takes the all-gather exchange below
                raise ValueError("attack 'fang_krum' needs whole client rows (row distances, not a coordinate-wise "
                                 "statistic): use exchange='allgather' (a rank's all-to-all slice is the whole "
                                 "matrix only at world 1)")
        if rcfg.attack == "fang_trim":
            seed = rcfg.attack_cfg.get("seed", rcfg.seed)
            if isinstance(seed, bool) or not isinstance(seed, int):
                raise ValueError(f"attack_cfg['seed'] must be an integer, got {seed!r}")
            self._fang_trim = (fang_trim_config(rcfg.num_clients, rcfg.num_attackers, rcfg.attack_cfg.get("b", 2.0)),
                               seed)
        defer = os.environ.get("FLR_DEFER_DEAD", "2")
        if defer == "1":  # loud: an old A/B script must not report numbers for another mode
            raise ValueError("FLR_DEFER_DEAD=1 (the dead-tap fill on a side stream beside the Krum chains) was "
                             "removed: measured slower in every variant (profiles/r6_dead/); use 0, or 2 (the default)")
        self.spec, self.rcfg, self.tcfg = spec, rcfg, tcfg
        self.device = torch.device(device)
        self.rank, self.world = rank, world
        K = rcfg.num_clients
        self.lo, self.hi = fdist.shard(K, world, rank)
        shapes = [s for _, s in param_layout(spec)]
        # the ResNet + GRU and ViT + BERT families train through one C entry
        # (flr_train_clients_ex / flr_train_vit_bert: no torch kernel in the
        # training phase); FLR_TRAINER=python: the autograd composition of the
        # same kernels (A/B; the CUB family)
        self.native = (spec.family in ("resnet_gru", "vit_bert") and self.device.type == "cuda"
                       and os.environ.get("FLR_TRAINER", "native") != "python")
        if self.native:
            from .native_trainer import NativeRoundTrainer
            self.trainer = NativeRoundTrainer(spec, self.hi - self.lo, self.device, tcfg, batch=rcfg.batch)
        else:
            self.trainer = ClientBatchTrainer(spec, self.hi - self.lo, self.device, tcfg)
        cfg = dict(rcfg.defense_cfg)
        if rcfg.defense in ("krum", "multi_krum", "krum_trimmed_mean", "bulyan"):  # run_experiments.py:155-162
            cfg.setdefault("num_malicious", rcfg.num_attackers)
            cfg.setdefault("multi_k", max(1, K // 2))
        elif rcfg.defense == "dnc":
            cfg.setdefault("num_malicious", rcfg.num_attackers)
        elif rcfg.defense == "robust_lr":  # the paper's guidance: the threshold exceeds the attacker count
            cfg.setdefault("threshold", min(K, rcfg.num_attackers + 1))
        self.defense = get_defense(rcfg.defense, cfg)
        mode = rcfg.exchange
        if mode == "auto":
            mode = "alltoall" if (self.defense.supports_sharded and PW_SLICES % world == 0
                                  and self._minmax is None and not self._replace_whole_rows
                                  and self._fang_krum is None) else "allgather"
        if mode not in ("alltoall", "allgather"):
            raise ValueError(f"unknown exchange mode {rcfg.exchange!r}")
        if mode == "alltoall" and not self.defense.supports_sharded:
            raise ValueError(f"{self.defense!r} needs whole client rows: use exchange='allgather'")
        self.exchange = mode
        self.xchg = None
        self._full = self._slice = None  # outside readers: the full / slice properties (they make X whole first)
        self.global_flat = initial_global(spec, rcfg.seed, self.device)
        steps = tcfg.local_steps
        self.batches = synthetic_batches(spec, steps, range(self.lo, self.hi), rcfg.batch, self.device)
        self.masks = make_dropout_masks(spec, steps, range(self.lo, self.hi), rcfg.batch, self.device,
                                        seed=rcfg.seed + 7919)
        # data poisoning of the malicious clients (run_experiments.py:173-175)
        if rcfg.attack in ("backdoor", "model_replacement"):
            cols = [c - self.lo for c in range(self.lo, min(self.hi, rcfg.num_attackers))]
            poison_batches_(self.batches, cols, Backdoor(image_size=(spec.image_size, spec.image_size)))
        self.num_examples = [steps * rcfg.batch] * K  # len(client dataset) (run_experiments.py:240)
        self.losses: Optional[torch.Tensor] = None
        self.use_graph = (rcfg.graph and self.device.type == "cuda" and os.environ.get("FLR_GRAPH", "1") != "0")
        self._graph = None
        self._graph_losses: Optional[torch.Tensor] = None
        # the defense takes the round's global model (its slice, for a rank's coordinate range)
        self._wants_global = self.defense.takes_global
        # training-order rounds (BaseDefense.order_free): the client matrix is in
        # the trainer's coordinate order, written by the last optimizer step;
        # gtrain is the global model in that order (FLR_ORDER=torch: off)
        # Min-Max / Min-Sum read the round's global model beside the matrix: torch
        # order, where global_flat lines up with the columns (model replacement and Fang et al.'s attacks likewise)
        self.train_order = (getattr(self.defense, "order_free", False) and not self._wants_global
                            and self._minmax is None and self._replace is None
                            and self._fang_krum is None and self._fang_trim is None
                            and os.environ.get("FLR_ORDER", "train") != "torch")
        bounds = None
        if self.train_order and getattr(self.defense, "needs_tap_blocks", False):
            # the reference-exact distances read the training-order matrix,
            # told which blocks are tap-major (no torch-order copy)
            ok, taps = self._tap_blocks()
            if ok and self.exchange == "alltoall" and world > 1:
                # the chains run through the ranks' coordinate ranges in torch
                # order: rank boundaries moved off the tap-major blocks, so each
                # range holds whole blocks (the same set in either order)
                bounds = aligned_bounds(self.trainer.P, world, taps)
                ok = bounds is not None
            self.train_order = ok
            self.defense.tap_blocks = taps if ok else None
        if mode == "alltoall":
            self.xchg = CoordExchange(K, self.hi - self.lo, self.trainer.P, self.device, Comm(), bounds=bounds)
        else:
            self._full = self.trainer.X if world == 1 else ClientMatrix.empty(K, shapes, self.device)
            if world > 1 and hasattr(self.defense, "comm"):
                # whole rows on every rank: the reference-exact Krum distances
                # split their pair tiles over the ranks (one 8·K² all-reduce)
                self.defense.comm = Comm()
        self.gtrain = self.trainer.to_train_order(self.global_flat) if self.train_order else None
        # FLR_DEFER_DEAD=2 (default): the dead-tap slabs (copies of the global
        # model, 58 % of P at C3) are not written by the round at all — the
        # distances read them from the round's global vector, the Multi-Krum
        # mean too (flr_rows_mean_dead): C3 15.65-15.73 -> 15.94-15.99 rounds/s,
        # the same bits (profiles/r6_dead/); materialize() writes them for any
        # other reader of X (the full / slice / client_matrix properties call
        # it); =0: written last in the training phase.  Not armed under the
        # colluding attacks (alie, ipm): their pass reads the benign rows and
        # writes the attackers' rows whole, before the defense (min_max, min_sum
        # likewise: they run in torch order, where nothing is deferred)
        self._dead: Optional[DeadTaps] = None
        self._x_stale = False  # set where run_round arms the deferral, cleared by materialize() alone
        if (self.train_order and world == 1 and self._collude is None and self.defense.__dict__.get("tap_blocks")
                and getattr(self.defense, "supports_dead_rows", False)
                and hasattr(self.trainer, "fill_dead") and defer == "2"):
            masks = self._dead_masks(self.defense.tap_blocks)
            if masks is not None and any(masks):
                self.trainer.defer_dead = True
                # g: the global vector the round trained from (gtrain is overwritten by the publish)
                self._dead = DeadTaps(masks, self.trainer.dead_ranges(),
                                      torch.empty(self.trainer.P, dtype=torch.float32, device=self.device),
                                      self._num_flipped())

        self.round_index = 0
        self.fell_back = False
        self.fallback_error: Optional[str] = None   # exception type of the last FedAvg fallback

    def _tap_blocks(self):
        """(ok, blocks): the training-order matrix's tap-major convolution
        weights [(off, Cout, Cin, KK), ...] (flr_pairwise_l2_reference_tap),
        checked once against the trainer's own reorder of a column-index
        vector (float32: exact below 2^24 coordinates; past that, or on any
        mismatch, ok=False: a torch-order round)."""
        from .models.multimodal import param_layout, tap_major_names
        P = self.trainer.P
        if P >= 1 << 24:
            return False, None
        tapn = tap_major_names(self.spec) if self.spec.family != "vit_bert" else frozenset()
        blocks, off = [], 0
        for name, shape in param_layout(self.spec):
            n = 1
            for d in shape:
                n *= int(d)
            if name in tapn:
                blocks.append((off, int(shape[0]), int(shape[1]), int(shape[2]) * int(shape[3])))
            off += n
        want = torch.arange(P, dtype=torch.int64, device=self.device)
        for o, co, ci, kk in blocks:
            u = torch.arange(co * ci * kk, dtype=torch.int64, device=self.device)
            want[o:o + co * ci * kk] = o + ((u % kk) * ci + (u // kk) % ci) * co + u // (ci * kk)
        got = self.trainer.to_torch_order(torch.arange(P, dtype=torch.float32, device=self.device))
        if not torch.equal(got.to(torch.int64), want):
            return False, None
        return True, blocks

    def _dead_masks(self, taps):
        """Per tap block the bitmask of its dead taps (the trainer's dead ranges,
        each a whole tap slab of one block), or None when a range is not (or a
        dead coordinate falls in the last P mod 8, which the distances read
        from X directly)."""
        ranges = self.trainer.dead_ranges()
        P = self.trainer.P
        masks = [0] * len(taps)
        for o, n in ranges:
            if o + n > P - P % 8:
                return None
            for b, (off, co, ci, kk) in enumerate(taps):
                slab = co * ci
                if off <= o and o + n <= off + kk * slab:
                    if (o - off) % slab or n % slab or kk > 64:
                        return None
                    for t in range((o - off) // slab, (o - off + n) // slab):
                        masks[b] |= 1 << t
                    break
            else:
                return None
        return masks

    def materialize(self) -> None:
        """X's dead-tap ranges written (FLR_DEFER_DEAD=2 leaves them out), from
        the global vector the last round trained from.  Idempotent; the
        full / slice / client_matrix properties call it."""
        if self._x_stale:
            self.trainer.fill_dead(self._dead.g, self._dead.nneg)
            self._x_stale = False

    @property
    def dead_deferred(self) -> bool:
        """The rounds leave X's dead-tap ranges unwritten (FLR_DEFER_DEAD=2)."""
        return self._dead is not None

    @property
    def client_matrix(self) -> ClientMatrix:
        """This rank's rows of the client matrix, whole: the supported way to
        read them (eng.trainer.X is the trainer's raw buffer, whose dead-tap
        ranges a round may have left unwritten)."""
        self.materialize()
        return self.trainer.X

    @property
    def full(self) -> Optional[ClientMatrix]:
        """The all-gather exchange's K×P matrix of the last round, whole."""
        self.materialize()
        return self._full

    @property
    def slice(self):
        """The all-to-all exchange's coordinate slice of the last round, whole."""
        self.materialize()
        return self._slice

    def _num_flipped(self) -> int:
        """Local rows of sign-flip attackers (clients 0..f-1): they submit
        -update, the weights negated as the reference does (model_poisoning.py:
        274-276 via malicious_client.py:103-115) — written negated by the export."""
        f = self.rcfg.num_attackers if self.rcfg.attack == "sign_flip" else 0
        return max(0, min(self.hi, f) - self.lo)

    def _train_phase(self) -> torch.Tensor:
        """Every local client: global -> local SGD steps -> client-matrix rows
        (run_experiments.py:193-240), the attackers' poisoning in the export."""
        if self.train_order:
            self.trainer.load_global_train(self.gtrain)
            return self.trainer.local_update(self.batches, self.masks, negate_rows=self._num_flipped(),
                                             gtrain=self.gtrain)
        self.trainer.load_global(self.global_flat)
        return self.trainer.local_update(self.batches, self.masks, negate_rows=self._num_flipped())

    def _publish(self, agg: Optional[torch.Tensor] = None) -> torch.Tensor:
        """The round's aggregate -> global_flat (torch order; and gtrain when
        training order is on, agg then being in training order)."""
        if self.train_order:
            if agg is not None:
                self.gtrain.copy_(agg)
            self.trainer.to_torch_order(self.gtrain, self.global_flat)
        elif agg is not None:
            self.global_flat.copy_(agg)
        self.round_index += 1
        return self.global_flat

    def _capture(self, keep_graph: bool = False) -> None:
        """Capture the training phase (~2.4k kernel launches per round at C3)
        as one HIP graph: replay removes the host launch cost, which dominates
        once a GPU holds few clients (K/G = 16 at 8 GPUs).  Inputs (global
        vector, batches, masks) and the training state live at fixed addresses,
        so the graph reads the current round's global model on every replay."""
        side = torch.cuda.Stream(self.device)
        side.wait_stream(torch.cuda.current_stream(self.device))
        with torch.cuda.stream(side):  # warm-up on a side stream: library handles and workspaces
            self._train_phase()
        torch.cuda.current_stream(self.device).wait_stream(side)
        g = torch.cuda.CUDAGraph(keep_graph=keep_graph)  # keep_graph: the raw graph stays queryable (tools)
        with torch.cuda.graph(g):
            self._graph_losses = self._train_phase()
        self._graph = g

    def run_round(self) -> torch.Tensor:
        if self.use_graph:
            if self._graph is None:
                self._capture()
            self._graph.replay()
            self.losses = self._graph_losses
        else:
            self.losses = self._train_phase()
        if self._dead is None:
            return self._aggregate_phase()
        # the training phase left X's dead-tap slabs out: the defense reads them
        # from this round's global vector, every other reader after materialize()
        _capi.call("flr_copy_rows", self.gtrain.data_ptr(), self.trainer.P, self.trainer.P, self._dead.g.data_ptr(),
                   self.trainer.P, 1, torch.cuda.current_stream(self.device).cuda_stream)
        self._x_stale = True
        self.defense.dead = self._dead
        try:
            return self._aggregate_phase()
        finally:
            self.defense.dead = None

    def _aggregate_phase(self) -> torch.Tensor:
        kw = {"publish": False} if hasattr(self.defense, "publish") else {}
        self.fell_back = False
        self.fallback_error = None
        if self.exchange == "alltoall":
            cs = self._slice = self.xchg.exchange(self.trainer.X.data)
            # coordinate-wise: this rank's slice needs no other
            self._apply_collusion(cs.X, self.global_flat[cs.begin:cs.end], cs.begin)
            if self._wants_global:  # the robust learning rate: global_flat is overwritten below
                kw["global_flat"] = self.global_flat[cs.begin:cs.end].clone()
            try:
                part = self.defense.aggregate_sharded(cs, self.num_examples, **kw)
            except Exception as e:  # noqa: BLE001 - the reference catches any exception
                part = self._fallback(e, cs.X)
            cs.gather_vector(part, self.gtrain if self.train_order else self.global_flat)
            return self._publish()
        fdist.allgather_rows(self.trainer.X.data, self._full.data)
        self._apply_collusion(self._full.X)  # replicated: every rank computes the same bits
        if self._wants_global:  # FLTrust: the server update starts from this round's global model
            kw["global_flat"] = self.global_flat.clone()  # global_flat is overwritten below
        try:
            agg = self.defense.aggregate_flat(self._full, self.num_examples, **kw)
        except Exception as e:  # noqa: BLE001
            agg = self._fallback(e, self._full.X)
        return self._publish(agg)

    def _apply_collusion(self, X: torch.Tensor, g: Optional[torch.Tensor] = None, col0: int = 0) -> None:
        """attack "alie" / "ipm" / "min_max" / "min_sum": the attackers (clients
        0..f-1, who trained honestly) replace their rows of the exchanged matrix
        by the colluding vector, computed from the benign rows — after the
        exchange, before the defense, outside the captured training graph.
        "model_replacement": they boost their own (backdoored) rows about the
        global model; g is global_flat, or its slice beside a rank's coordinate
        range (stealth "none" alone runs there: it is coordinate-wise).
        "fang_krum" / "fang_trim": Fang et al.'s attacks in the same slot;
        fang_trim is coordinate-wise and runs on a rank's range too, its draws
        keyed by the coordinate's index in the order the matrix is held in
        (col0 + the column: torch order, col0 the range's first coordinate),
        the attacker and the round counter."""
        if self._collude is not None:
            ops.collude_rows(X, self.rcfg.num_attackers, *self._collude)
        if self._minmax is not None:  # global_flat: still the model this round trained from
            self.attack_gamma = ops.minmax_rows(X, self.rcfg.num_attackers, *self._minmax, self.global_flat)
        if self._replace is not None:
            self.attack_gamma, self.attack_status, self.attack_flags = replace_rows_(
                X, self.rcfg.num_attackers, self.global_flat if g is None else g, *self._replace)
        if self._fang_krum is not None:
            self.attack_gamma, self.attack_status = ops.fang_krum_rows(X, self.rcfg.num_attackers, self.global_flat,
                                                                       self._fang_krum)
        if self._fang_trim is not None:
            b, seed = self._fang_trim
            ops.fang_trim_rows(X, self.rcfg.num_attackers, (self.global_flat if g is None else g).contiguous(), b,
                               seed, self.round_index % 2 ** 32, col0)

    def _fallback(self, err: Exception, X: torch.Tensor) -> torch.Tensor:
        """robust_server.py:120-122: a failing defense falls back to FedAvg
        (only with RoundConfig.fallback_fedavg; otherwise the error propagates).
        The reference catches every Exception; RoundConfig.fallback_device_errors
        = False keeps device / library failures (kernel launch, workspace, HIP or
        RCCL errors, out of memory) loud instead."""
        device_error = isinstance(err, (_capi.FlrError, torch.cuda.OutOfMemoryError))
        if not self.rcfg.fallback_fedavg or (device_error and (not self.rcfg.fallback_device_errors
                                                               or self.world > 1)):
            raise err  # decided before anything is launched: the defense's own error propagates
        logging.getLogger(__name__).error("Defense aggregation failed: %s, falling back to FedAvg", err)
        self.fell_back = True
        self.fallback_error = type(err).__name__
        self.materialize()  # FedAvg reads whole rows
        return ops.fedavg(X, self.num_examples)

    # ---- checkpoint / resume (run_experiments.py:268-279) ----------------------
    def state_dict(self) -> Dict[str, torch.Tensor]:
        """The global model's state_dict: parameters() from the global vector,
        buffers (BatchNorm running statistics) at their initial values — the
        simulation never updates the global model's buffers (:257-259)."""
        m = model_class(self.spec)(self.spec)
        flat = self.global_flat.detach().cpu()
        off = 0
        with torch.no_grad():
            for p in m.parameters():
                n = p.numel()
                p.copy_(flat[off:off + n].view(p.shape))
                off += n
        return m.state_dict()

    def save_checkpoint(self, path: str, accuracy: Optional[float] = None, loss: Optional[float] = None) -> None:
        """torch.save({'round', 'model_state_dict', 'accuracy', 'loss'}) — the
        reference's checkpoint dict (run_experiments.py:273-279)."""
        torch.save({"round": self.round_index, "model_state_dict": self.state_dict(), "accuracy": accuracy,
                    "loss": loss}, path)

    def load_checkpoint(self, path: str) -> int:
        """Resume: the global vector and round index from save_checkpoint's file
        (weights_only load: nothing in the file is executed)."""
        ck = torch.load(path, map_location="cpu", weights_only=True)
        names = [n for n, _ in param_layout(self.spec)]
        sd = ck["model_state_dict"]
        flat = torch.cat([sd[n].reshape(-1).float() for n in names])
        self.global_flat.copy_(flat.to(self.global_flat.device))
        if self.train_order:
            self.gtrain.copy_(self.trainer.to_train_order(self.global_flat))
        self.round_index = int(ck["round"])
        return self.round_index

    # ---- per-round evaluation (run_experiments.py:261-266, 281-291) ------------
    def evaluator(self):
        """The GlobalEvaluator (flr.metrics) of this engine's model, created on
        first use; evaluate the current global model with
        ``eng.evaluator().load(eng.global_flat)`` then ``evaluate_model(...)`` /
        ``attack_success_rate(...)``."""
        if getattr(self, "_evaluator", None) is None:
            from .metrics import GlobalEvaluator
            self._evaluator = GlobalEvaluator(self.spec, self.device, batch_size=self.rcfg.batch)
        return self._evaluator

    def evaluate(self, images, text, labels):
        """evaluate_model(global_model, test_loader) of the reference's round
        loop (run_experiments.py:262) on the current global model."""
        ev = self.evaluator()
        ev.load(self.global_flat)
        return ev.evaluate_model(images, text, labels)
