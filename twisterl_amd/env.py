"""`twisterl.env` surface: Puzzle with the PyBaseEnv methods.

Mirrors reference rust/src/python_interface/env.rs:39-160 (PyBaseEnv + Puzzle) over
rust/src/envs/puzzle.rs.  The object is a host-side handle owned by libtwisterl_hip.so
(tw_puzzle_*); collectors read only its descriptor -- like the reference, which clones and
resets the env per episode and never mutates the one passed in (collector/ppo.rs:59-60).
"""
from __future__ import annotations

import ctypes as C

from . import _lib


class PyBaseEnv:
    """Base class of envs the HIP collectors accept (python_interface/env.rs:39-114)."""

    _h = None

    def __del__(self):
        h, self._h = getattr(self, "_h", None), None
        if h:
            try:
                _lib.lib().tw_puzzle_destroy(h)
            except Exception:
                pass

    # -- PyBaseEnv pymethods (env.rs:44-114) ---------------------------------------------------
    def num_actions(self) -> int:
        return int(_lib.lib().tw_puzzle_num_actions(self._h))

    def obs_shape(self) -> list:
        out = (C.c_uint32 * 2)()
        _lib.check(_lib.lib().tw_puzzle_obs_shape(self._h, out))
        return [int(out[0]), int(out[1])]

    @property
    def difficulty(self) -> int:
        return int(_lib.lib().tw_puzzle_get_difficulty(self._h))

    @difficulty.setter
    def difficulty(self, value: int) -> None:
        if int(value) < 0:
            raise OverflowError("can't convert negative int to unsigned")
        _lib.check(_lib.lib().tw_puzzle_set_difficulty(self._h, int(value)))

    def set_state(self, state) -> None:
        arr = (C.c_int64 * len(state))(*[int(s) for s in state])
        _lib.check(_lib.lib().tw_puzzle_set_state(self._h, arr, len(state)))

    def reset(self, seed: int = None, episode: int = 0) -> None:
        """Scramble by `difficulty` uniform moves (puzzle.rs:119-133).  The reference draws from
        the unseedable thread_rng; here the draw is stream 0 of the library's counter-based RNG,
        keyed by (seed, episode).  seed=None picks a fresh OS seed, like the reference."""
        if seed is None:
            import os
            seed = int.from_bytes(os.urandom(8), "little")
        _lib.check(_lib.lib().tw_puzzle_reset(self._h, int(seed) & (2**64 - 1), int(episode)))

    def step(self, action: int) -> None:
        _lib.check(_lib.lib().tw_puzzle_step(self._h, int(action)))

    def masks(self) -> list:
        out = (C.c_uint8 * 4)()
        _lib.check(_lib.lib().tw_puzzle_masks(self._h, out))
        return [bool(x) for x in out]

    def is_final(self) -> bool:
        return bool(_lib.lib().tw_puzzle_is_final(self._h))

    def reward(self) -> float:
        return float(_lib.lib().tw_puzzle_reward(self._h))

    def observe(self) -> list:
        n = self.obs_shape()[0]
        out = (C.c_int64 * n)()
        _lib.check(_lib.lib().tw_puzzle_observe(self._h, out))
        return [int(x) for x in out]

    def twists(self):
        """Env::twists default (rl/env.rs:59): Puzzle does not override it."""
        return ([], [])

    def __extract_env__(self) -> int:
        """Address of the native env object (env.rs:109-113).  Here it is a `tw_puzzle*` of
        libtwisterl_hip.so, not a Rust Box<dyn Env>."""
        return int(self._h)

    # -- used by the collectors ----------------------------------------------------------------
    def _desc(self) -> "_lib.PuzzleDesc":
        d = _lib.PuzzleDesc()
        _lib.check(_lib.lib().tw_puzzle_get_desc(self._h, C.byref(d)))
        return d


class Puzzle(PyBaseEnv):
    """Puzzle(width, height, difficulty, depth_slope, max_depth) (env.rs:117-160)."""

    def __init__(self, width: int, height: int, difficulty: int, depth_slope: int, max_depth: int):
        for v in (width, height, difficulty, depth_slope, max_depth):
            if int(v) < 0:
                raise OverflowError("can't convert negative int to unsigned")
        self._h = _lib.lib().tw_puzzle_create(int(width), int(height), int(difficulty), int(depth_slope),
                                              int(max_depth))
        if not self._h:
            raise ValueError(_lib.last_error())

    def solved(self) -> bool:
        return bool(_lib.lib().tw_puzzle_solved(self._h))

    def get_state(self) -> list:
        n = self.obs_shape()[0]
        out = (C.c_int64 * n)()
        _lib.check(_lib.lib().tw_puzzle_get_state(self._h, out))
        return [int(x) for x in out]

    def display(self) -> None:
        """puzzle.rs:56-69"""
        w = int(self._desc().width)
        line = ""
        for i, v in enumerate(self.get_state()):
            line += "   " if v == 0 else (f"  {v} " if v < 10 else f" {v} ")
            if (i + 1) % w == 0:
                print(line)
                line = ""

    def set_position(self, x: int, y: int, val: int) -> None:
        _lib.check(_lib.lib().tw_puzzle_set_position(self._h, int(x), int(y), int(val)))

    def get_position(self, x: int, y: int) -> int:
        return int(_lib.lib().tw_puzzle_get_position(self._h, int(x), int(y)))

    @property
    def depth(self) -> int:
        return int(_lib.lib().tw_puzzle_depth(self._h))


class PyEnv:
    """PyEnv(pyenv): an environment implemented in Python (reference rust/src/python_interface/pyenv.rs:41-160,
    src/twisterl/envs/__init__.py:20-25).  `pyenv` provides the methods the reference calls on it: copy(), num_actions(),
    obs_shape(), reset(difficulty), next(action), masks(), is_final(), value(), success(), observe(), set_state(state).
    Its code runs on the host -- as in the reference -- while the policy forward of all live episodes of a time step is one
    batched launch on the GPU (tw_ppo_collect_env).  Build extension: if `pyenv` has seed_episode(seed, episode) it is
    called before every reset(), so that a collect is reproducible (the reference's envs draw from OS entropy).
    Observation length: by default observe() must return the SAME NUMBER of ids for every state (the prototype's) and masks()
    one flag per action -- the C side's per-state buffers have that size (tw_env_vtable.n_obs).  An environment whose
    observations vary in length, which the reference's EmbeddingBag takes as they come (layers.rs:56-62), says so by defining
    max_obs() -> the largest number of ids any state returns, 1..64 (build extension, like seed_episode): observe() may then
    return 0 .. max_obs() ids, the policy sums the vectors of exactly those, and the collected `.obs` is a list of lists of
    differing length (the device buffer: dense uint16 rows, 0xFFFF in the free slots -- CollectedData).  A length above
    max_obs(), a changing length without max_obs(), or an id outside obs_shape raises from collect() / evaluate() / solve()."""

    def __init__(self, pyenv):
        for m in ("copy", "num_actions", "obs_shape", "reset", "next", "masks", "is_final", "value", "observe"):
            if not callable(getattr(pyenv, m, None)):
                raise TypeError(f"PyEnv: the environment object has no method {m}()")
        self._env = pyenv
        self._difficulty = 1                                   # PyEnvImpl::new (pyenv.rs:41-45)

    def __extract_env__(self) -> int:
        return id(self)

    difficulty = property(lambda self: self._difficulty, lambda self, d: setattr(self, "_difficulty", int(d)))

    def num_actions(self) -> int:
        return int(self._env.num_actions())

    def obs_shape(self) -> list:
        return [int(x) for x in self._env.obs_shape()]

    def set_state(self, state) -> None:
        self._env.set_state([int(x) for x in state])

    def reset(self) -> None:
        self._env.reset(self._difficulty)

    def step(self, action: int) -> None:
        self._env.next(int(action))

    def masks(self) -> list:
        return [bool(m) for m in self._env.masks()]

    def is_final(self) -> bool:
        return bool(self._env.is_final())

    def reward(self) -> float:
        return float(self._env.value())

    def observe(self) -> list:
        return [int(x) for x in self._env.observe()]

    def twists(self):
        """Env::twists (rl/env.rs:58-59).  The reference's PyEnvImpl keeps the trait's default (no twists); a Python environment
        that defines twists() is honoured here (build extension) -- the host builds its Policy with them."""
        if callable(getattr(self._env, "twists", None)):
            op, ap = self._env.twists()
            return [[int(x) for x in p] for p in op], [[int(x) for x in p] for p in ap]
        return ([], [])

    def track_solution(self) -> bool:
        """Env::track_solution (rl/env.rs:62): false unless the Python environment says otherwise (build extension)."""
        return bool(self._env.track_solution()) if callable(getattr(self._env, "track_solution", None)) else False

    def solution(self) -> list:
        """Env::solution (rl/env.rs:65)."""
        return [int(x) for x in self._env.solution()] if callable(getattr(self._env, "solution", None)) else []


def get_env_desc(py_env) -> "_lib.PuzzleDesc":
    """Counterpart of get_env() (env.rs:163-177).  The reference turns the integer returned by
    `__extract_env__` back into a Rust Box<dyn Env>; this library can only run envs whose
    dynamics it implements on the GPU, so the object must be one of ours."""
    if not hasattr(py_env, "__extract_env__"):
        raise TypeError("Object must implement __extract_env__ method")
    if isinstance(py_env, PyEnv):
        raise TypeError("environments implemented in Python are collected by PPOCollector (tw_ppo_collect_env); self-play, "
                        "evaluate and solve run environments whose dynamics the library implements on the GPU (Puzzle)")
    if not isinstance(py_env, PyBaseEnv):
        raise TypeError("Expected environment of type twisterl_amd.env.Puzzle "
                        "(the HIP collectors cannot run a foreign Box<dyn Env>)")
    return py_env._desc()


class DeviceEnvDesc(C.Structure):
    """struct tw_device_env (twisterl_amd/csrc/tw_rollout_env.hpp): what a device-environment module exports."""
    _fields_ = [("layout", C.c_uint32 * 8), ("num_actions", C.c_uint32), ("n_obs", C.c_uint32), ("state_bytes", C.c_uint32),
                ("engine_nc", C.c_uint32), ("type_name", C.c_char_p), ("launch_rollout", C.c_void_p), ("launch_solve", C.c_void_p),
                ("create", C.CFUNCTYPE(C.c_void_p, C.POINTER(C.c_double), C.c_int)),
                ("get_difficulty", C.CFUNCTYPE(C.c_int, C.c_void_p)), ("set_difficulty", C.CFUNCTYPE(None, C.c_void_p, C.c_int)),
                ("obs_size", C.CFUNCTYPE(C.c_int, C.c_void_p)), ("n_obs_of", C.CFUNCTYPE(C.c_int, C.c_void_p)), ("fill_vtable", C.c_void_p),
                ("launch_search", C.c_void_p),
                ("groups_per_cu", C.CFUNCTYPE(C.c_int, C.c_int, C.c_size_t, C.POINTER(C.c_int))),
                ("launch_rollout16", C.c_void_p), ("groups_per_cu16", C.CFUNCTYPE(C.c_int, C.c_size_t, C.POINTER(C.c_int)))]


class DeviceEnv:
    """DeviceEnv(module_path, name, params=[...]): a user-written environment that runs ON THE DEVICE -- a C++ struct
    (include/twisterl_device_env.hpp) compiled by twisterl_amd.build.build_device_env into `module_path`, which exports
    tw_device_env_<name>.  `params` go to the struct's init() (the environment's constructor arguments).

    PPOCollector.collect and evaluate run its episodes inside one kernel each (tw_ppo_collect_device_env / tw_evaluate_device_env);
    a module built with build_device_env(..., fp16=True) also runs PPOCollector(precision="fp16").collect in one kernel, every Linear
    of any generic policy on the f16 matrix core (`fp16` says whether the module has that kernel; without it: "f32 only"), and one
    built with fp16_solve=True runs collector.evaluate / collector.solve with precision="fp16" and no MCTS likewise (`fp16_solve`),
    one built with fp16_search=True beside a search form AZCollector(precision="fp16").collect and evaluate / solve WITH MCTS (`fp16_search`),
    one built with fp16x2=True PPOCollector(precision="fp16x2").collect, f32 answers from split binary16 operands (`fp16x2`),
    one built with fp16x2_solve=True collector.evaluate / collector.solve with precision="fp16x2" and no MCTS as well (`fp16x2_solve`);
    a policy of ONE common layer of 32 / 64 / 128 / 256 units with obs_size <= 256 (the reference's default) runs host-stepped in all
    of these unless the module was built with basic=True (`basic`), which takes it into the f32 kernels;
    a module built with build_device_env(..., search=True) (1..4 actions; wide_search=True: 1..31) runs AZCollector.collect and evaluate with MCTS inside one kernel too
    (tw_az_collect_device_env; `search` says whether the module has that kernel), any other module steps the same struct's host
    code for those (tw_az_collect_env / tw_evaluate_env).  solve runs from the object's CURRENT state in one kernel as evaluate does
    (tw_solve_device_env; with MCTS: a search module, else the host code, tw_solve_env32).  The object itself is a
    host copy of the struct with the PyBaseEnv surface (reset / step / masks / observe / reward / is_final); collectors clone
    it and reset the clones, as the reference does (collector/ppo.rs:59-60).

    `max_records`: the longest episode a collect accepts (a longer one fails it, as on the host-stepped path).  Set it to the
    environment's own bound (GridWorld: max_steps + 1): the device collect's padded workspace holds num_episodes x max_records x
    (48 + 2 x n_obs) bytes (n_obs: the longest observation, for a struct with observe_n) -- 65,536 GridWorld 5 x 5 episodes at the
    default 256: 1.6 GB.  Above 1,820 records the collect runs on
    the host-stepped path (the finalize step's LDS tile)."""

    def __init__(self, module_path: str, name: str, params=(), *, max_records: int = 256):
        import os
        L = _lib.lib()                           # (loads the HIP runtime torch uses first; the module binds to it)
        path = os.path.abspath(module_path)
        try:
            self._mod = C.CDLL(path)
        except OSError as e:
            raise RuntimeError(f"cannot load the device environment module {path}: {e}") from e
        fn = getattr(self._mod, f"tw_device_env_{name}", None)
        if fn is None:
            raise ValueError(f"{path} exports no tw_device_env_{name}")
        fn.restype, fn.argtypes = C.c_void_p, []
        self._desc_ptr = fn()
        self._desc = DeviceEnvDesc.from_address(self._desc_ptr)
        p = [float(x) for x in params]
        self._obj = self._desc.create((C.c_double * max(len(p), 1))(*p), len(p))
        if not self._obj:
            raise ValueError(f"{self._desc.type_name.decode()}: init() refused the parameters {p}")
        self._vt = _lib.EnvVTable()
        rc = L.tw_device_env_host_vtable(self._desc_ptr, self._obj, self._desc.state_bytes, C.byref(self._vt))
        if rc != _lib.TW_OK:
            msg = _lib.last_error()
            self._free()
            raise ValueError(msg)
        self.max_records = int(max_records)
        if not 1 <= self.max_records <= 0x7fffffff:
            raise ValueError("max_records must be positive")

    def _free(self):
        obj, self._obj = getattr(self, "_obj", None), None
        if obj:
            # the module's destroy (the vtable may not be filled yet: free through the one the module fills)
            vt = _lib.EnvVTable()
            C.CFUNCTYPE(None, C.POINTER(_lib.EnvVTable))(self._desc.fill_vtable)(C.byref(vt))
            vt.destroy(obj)

    def __del__(self):
        try:
            self._free()
        except Exception:
            pass

    # -- PyBaseEnv surface on the host copy ------------------------------------------------------
    @property
    def name(self) -> str:
        return self._desc.type_name.decode()

    def num_actions(self) -> int:
        return int(self._desc.num_actions)

    @property
    def n_obs(self) -> int:
        return int(self._vt.n_obs)                # (this object's: a struct with its own n_obs() may write fewer than N_OBS)

    @property
    def obs_size(self) -> int:
        return int(self._desc.obs_size(self._obj))

    @property
    def search(self) -> bool:
        """The module holds the search kernel (built with search=True or wide_search=True): self-play and MCTS-guided evaluate run on the device."""
        return bool(self._desc.launch_search)

    @property
    def fp16(self) -> bool:
        """The module holds the f16 rollout kernel (built with fp16=True): PPOCollector(precision="fp16").collect runs on the device."""
        return bool(self._desc.launch_rollout16)

    @property
    def fp16_solve(self) -> bool:
        """The module holds the f16 evaluate kernel (built with fp16_solve=True): collector.evaluate and collector.solve with
        precision="fp16" and no MCTS run on the device.  Asked of the module itself -- groups_per_cu(3, 0, null), which touches no
        device -- so it works on a machine without a GPU."""
        return int(self._desc.groups_per_cu(3, 0, None)) == 0

    @property
    def fp16_search(self) -> bool:
        """The module holds the f16 search kernel (built with fp16_search=True beside search=True or wide_search=True):
        AZCollector(precision="fp16").collect and collector.evaluate / collector.solve with MCTS and precision="fp16" run on the
        device.  Asked like fp16_solve -- groups_per_cu(4, 0, null) -- so it works on a machine without a GPU."""
        return int(self._desc.groups_per_cu(4, 0, None)) == 0

    @property
    def fp16x2(self) -> bool:
        """The module holds the split-f16 rollout kernel (built with fp16x2=True): PPOCollector(precision="fp16x2").collect runs on
        the device, f32 answers from split binary16 operands on the f16 matrix core.  Asked like fp16_solve -- groups_per_cu(5, 0,
        null) -- so it works on a machine without a GPU."""
        return int(self._desc.groups_per_cu(5, 0, None)) == 0

    @property
    def fp16x2_solve(self) -> bool:
        """The module holds the split-f16 evaluate kernel (built with fp16x2_solve=True): collector.evaluate and collector.solve with
        precision="fp16x2" and no MCTS run on the device, f32 answers from split binary16 operands.  Asked like fp16_solve --
        groups_per_cu(6, 0, null) -- so it works on a machine without a GPU."""
        return int(self._desc.groups_per_cu(6, 0, None)) == 0

    @property
    def basic(self) -> bool:
        """The module holds the kernel that packs the EngineV layers of a one-common-layer policy (built with basic=True): under the
        reference's default policy -- one common layer of 32 / 64 / 128 / 256 units, obs_size <= 256 -- the module's f32 kernels run
        on the device instead of the host-stepped path.  Asked like fp16_solve -- groups_per_cu(7, 0, null) -- so it works on a
        machine without a GPU."""
        return int(self._desc.groups_per_cu(7, 0, None)) == 0

    @property
    def variable_obs(self) -> bool:
        """The struct defines observe_n(): its observations hold 0 .. n_obs ids."""
        return bool(self._vt.observe_n)

    def obs_shape(self) -> list:
        """[n_obs, obs_size / n_obs] when that divides (GridWorld: [w*h, w*h], lib.rs obs_shape), else [obs_size]; [obs_size] for
        an environment whose observations vary in length (n_obs is then only their maximum)."""
        n, s = self.n_obs, self.obs_size
        return [n, s // n] if s % n == 0 and not self.variable_obs else [s]

    @property
    def difficulty(self) -> int:
        return int(self._desc.get_difficulty(self._obj))

    @difficulty.setter
    def difficulty(self, value: int) -> None:
        if int(value) < 0:
            raise OverflowError("can't convert negative int to unsigned")
        self._desc.set_difficulty(self._obj, int(value))

    def reset(self, seed: int = None, episode: int = 0) -> None:
        """Env::reset keyed by (seed, episode) as in the collectors; seed=None picks a fresh OS seed."""
        if seed is None:
            import os
            seed = int.from_bytes(os.urandom(8), "little")
        self._vt.reset(self._obj, int(seed) & (2**64 - 1), int(episode) & (2**64 - 1))

    def step(self, action: int) -> None:
        if not 0 <= int(action) < self.num_actions():
            raise ValueError(f"action {action} outside [0, {self.num_actions()})")
        self._vt.step(self._obj, int(action))

    def masks(self) -> list:
        out = (C.c_uint8 * self.num_actions())()
        self._vt.masks(self._obj, out)
        return [bool(x) for x in out]

    def observe(self) -> list:
        out = (C.c_int32 * self.n_obs)()
        if self.variable_obs:                     # the ids this state has
            k = int(self._vt.observe_n(self._obj, out, self.n_obs))
            if k > self.n_obs:
                raise ValueError(f"observation of {k} ids, at most {self.n_obs}")
            return [int(x) for x in out[:k]]
        self._vt.observe(self._obj, out)
        return [int(x) for x in out]

    def reward(self) -> float:
        return float(self._vt.reward(self._obj))

    def is_final(self) -> bool:
        return bool(self._vt.is_final(self._obj))

    def success(self) -> bool:
        return bool(self._vt.success(self._obj))

    def twists(self):
        """Env::twists default (rl/env.rs:59): none; a policy with twists is built by the host, as for any environment."""
        return ([], [])

    def state_bytes(self) -> bytes:
        """The struct as it is (it is trivially copyable: this IS the environment's state)."""
        return C.string_at(self._obj, self._desc.state_bytes)

    def set_state_bytes(self, data: bytes) -> None:
        if len(data) != self._desc.state_bytes:
            raise ValueError(f"{len(data)} bytes for a {self._desc.state_bytes}-byte environment")
        C.memmove(self._obj, bytes(data), len(data))

    def __extract_env__(self) -> int:
        """Address of the host copy of the struct (the prototype the collectors clone)."""
        return int(self._obj)

    # -- used by the collectors ------------------------------------------------------------------
    def _args(self):
        return self._desc_ptr, self._obj, self._desc.state_bytes
