"""Ring buffer of search self-play records (the rule: include/mnk_hip.h, mnk_search_selfplay_step / mnk_search_gather).

A record is one position of a self-play game with the root visit counts the search spent on it and, once the game has
ended, its outcome z from the view of the side to move there.  The ring holds ``capacity`` plies of ``num_envs`` rows:

    planes  int64 [T, 2, W, N]  packed canonical planes (PackedRolloutBuffer's layout: 16*W B per record)
    visits  int16 [T, N, C]     root visits (bit patterns of u16)
    z       int8  [T, N]        +1 / -1 / 0, or mnk_hip.Z_UNKNOWN while the game runs

``selfplay.search_selfplay.SearchSelfPlay`` writes it, one ``mnk_search_selfplay_step`` launch per ply; ``sample`` expands
a minibatch under the board's symmetries with one ``mnk_search_gather`` launch.  The count of plies written lives in a
device word (``plies``), so a captured self-play ply advances it too.
"""
from typing import Dict, Optional

import torch

import mnk_hip


class SearchReplayBuffer:
    def __init__(self, capacity: int, num_envs: int, m: int, n: int, device="cuda"):
        self.m, self.n, self.num_envs, self.capacity = int(m), int(n), int(num_envs), int(capacity)
        self.C = self.m * self.n
        if self.num_envs < 1:
            raise ValueError(f"num_envs must be >= 1, got {num_envs}")
        self.W = mnk_hip.state_words(self.m, self.n)
        if self.W == 0 or self.n < 2:
            raise ValueError(f"unsupported board {self.m}x{self.n}")
        if self.capacity < self.C:
            raise ValueError(f"capacity must be at least m*n = {self.C} plies (a game never wraps onto its own "
                             f"records), got {capacity}")
        self.device = torch.device(device)
        T, N, C = self.capacity, self.num_envs, self.C
        self.planes = torch.zeros((T, 2, self.W, N), dtype=torch.int64, device=self.device)
        self.visits = torch.zeros((T, N, C), dtype=torch.int16, device=self.device)
        self.z = torch.full((T, N), mnk_hip.Z_UNKNOWN, dtype=torch.int8, device=self.device)
        self.plies = torch.zeros(1, dtype=torch.int64, device=self.device)  # plies written (the step kernels' step_dev)
        self.plies_host = 0  # the same, as far as the host has launched them (eager plies and noted replays)
        self.err = torch.zeros(2, dtype=torch.int32, device=self.device)

    @property
    def symmetries(self) -> int:
        """the number of symmetries of the board: 8 when square, else 4"""
        return 8 if self.m == self.n else 4

    def sample(self, batch_size: int, symmetries: bool = True, obs_dtype=torch.float32,
               generator: Optional[torch.Generator] = None) -> Dict[str, torch.Tensor]:
        """``batch_size`` records drawn uniformly over the rows written so far, each under a symmetry drawn uniformly
        (``symmetries=False``: the identity).  Returns ``observation`` [B, 2, m, n] of ``obs_dtype`` (channel 0 = the side
        to move), ``action_mask`` bool [B, C], ``policy`` f32 [B, C] (the visit distribution), ``value`` f32 [B] (z) and
        ``weight`` f32 [B] (0 for records of games still running).  One gather launch; no host synchronisation."""
        B = int(batch_size)
        if B < 1:
            raise ValueError(f"batch_size must be >= 1, got {batch_size}")
        if self.plies_host == 0:
            raise ValueError("the buffer is empty")
        code = mnk_hip.obs_dtype_code(obs_dtype)
        dev = self.device
        filled = torch.clamp(self.plies, max=self.capacity) * self.num_envs  # (device word: capturable, no sync)
        u = torch.rand(B, dtype=torch.float64, device=dev, generator=generator)
        idx = torch.minimum((u * filled).to(torch.int64), filled - 1)
        sym = None
        if symmetries:
            sym = torch.randint(0, self.symmetries, (B,), dtype=torch.int8, device=dev, generator=generator)
        out = {"observation": torch.empty((B, 2, self.m, self.n), dtype=obs_dtype, device=dev),
               "action_mask": torch.empty((B, self.C), dtype=torch.bool, device=dev),
               "policy": torch.empty((B, self.C), dtype=torch.float32, device=dev),
               "value": torch.empty(B, dtype=torch.float32, device=dev),
               "weight": torch.empty(B, dtype=torch.float32, device=dev)}
        self.gather(idx, sym, out, code)
        return out

    def gather(self, idx: torch.Tensor, sym: Optional[torch.Tensor], out: Dict[str, torch.Tensor], obs_code=None):
        """the records of flat ids ``idx`` (int64 [B], t*N + i) under symmetries ``sym`` (int8 [B] or None) into the
        tensors of ``out`` (the keys of ``sample``; any may be missing)"""
        obs = out.get("observation")
        code = mnk_hip.obs_code(obs) if obs_code is None else obs_code
        mnk_hip.call("mnk_search_gather", mnk_hip.ptr(self.planes), mnk_hip.ptr(self.visits), mnk_hip.ptr(self.z),
                     self.capacity, self.num_envs, self.m, self.n, mnk_hip.ptr(idx), mnk_hip.ptr(sym), idx.numel(),
                     mnk_hip.ptr(obs), code, mnk_hip.ptr(out.get("action_mask")), mnk_hip.ptr(out.get("policy")),
                     mnk_hip.ptr(out.get("value")), mnk_hip.ptr(out.get("weight")), mnk_hip.ptr(self.err),
                     mnk_hip.stream_ptr(self.device))

    def check_errors(self) -> None:
        """raises on a sticky device error of a gather (one synchronisation)"""
        code, where = self.err.tolist()
        if code:
            self.err.zero_()
            raise IndexError(f"search gather: device error {code} at sample {where}")

    def state_dict(self) -> Dict[str, torch.Tensor]:
        return {"geometry": torch.tensor([self.capacity, self.num_envs, self.m, self.n]), "planes": self.planes.cpu(),
                "visits": self.visits.cpu(), "z": self.z.cpu(), "plies": self.plies.cpu()}

    def load_state_dict(self, state: Dict[str, torch.Tensor]) -> None:
        if state["geometry"].tolist() != [self.capacity, self.num_envs, self.m, self.n]:
            raise ValueError(f"state is for {state['geometry'].tolist()}, this buffer is "
                             f"{[self.capacity, self.num_envs, self.m, self.n]}")
        self.planes.copy_(state["planes"])
        self.visits.copy_(state["visits"])
        self.z.copy_(state["z"])
        self.plies.copy_(state["plies"])
        self.plies_host = int(state["plies"].item())
        self.err.zero_()
