"""Scenes in which a satellite leaves and returns, for the receiver-lifecycle tests -- TEST INFRASTRUCTURE ONLY.

`render_with_presence` renders every satellite of a `synth.SyntheticScene` on its own without noise, switches it on and off per
millisecond with a 0/1 mask, and adds one noise-only render of the same seed: with all-ones masks that is `synth.render(scene)` up
to the float32 rounding of the parts (tests/test_receiver_model.py asserts it).

R1, R2, R3 are the three scenes of tests/test_receiver_model.py (R2) and tests/test_gpu_receiver_lifecycle.py (all three):
satellite X (the scene's first) is absent for `absent_ms`, is dropped by the circularity watchdog, goes back on the search list and is
acquired again by a later scan.  `scene_conditions` states what a scene must show IN THE FLOAT64 MODEL ALONE before a device
result is compared with it.
"""
from __future__ import annotations

import dataclasses
from dataclasses import dataclass
from typing import Dict, List, Optional, Tuple

import numpy as np

from gypsum_amd import synth
from oracle import gypsum_oracle as orc


def render_with_presence(scene: synth.SyntheticScene, presence: Dict[int, np.ndarray]) -> np.ndarray:
    """complex64[n_ms * N]; presence[sat_id]: n_ms values in {0, 1} (a satellite without an entry is present throughout)."""
    n = scene.samples_per_ms
    acc = synth.render(dataclasses.replace(scene, sats=[])).astype(np.complex128)              # the scene's noise alone
    for s in scene.sats:
        part = synth.render(dataclasses.replace(scene, sats=[s], noise_sigma=0.0)).astype(np.complex128)
        mask = presence.get(s.sat_id)
        if mask is not None:
            mask = np.asarray(mask)
            if mask.shape != (scene.n_ms,) or not np.isin(mask, (0, 1)).all():
                raise ValueError("a presence mask holds one 0 or 1 per millisecond")
            part *= np.repeat(mask.astype(np.float64), n)
        acc += part
    return acc.astype(np.complex64)


@dataclass(frozen=True)
class LifecycleScene:
    name: str
    fs: int
    n_ms: int
    n_sats: int
    seed: int
    absent_ms: Tuple[int, int]            # X is absent during milliseconds [from, to)
    n_absent_on_list: int                 # satellites on the search list that are not in the scene at all
    scan_period_s: float                  # ACQUISITION_SCAN_FREQUENCY (config.py:9: 10)
    watchdog_period_s: float              # tracker.py:372: 6

    def scene(self) -> synth.SyntheticScene:
        """`n_sats` satellites with amplitudes inside synth.lock_regime_scene's ranges (a*N in 14..27, per-component noise variance of
        the prompt peak v in 0.05..1.7), from the part of them where a channel locks firmly once its window has filled: a*N ~ U(20, 27)
        and v ~ U(0.05, 0.6), so (a*N)^2 v < 440 against the lock test's 900 -- a channel that flaps about a threshold for seconds
        comes within 1e-5 of it sooner or later, which the conditions below rule out."""
        rng = np.random.default_rng([self.seed, 0x1EAF])
        n = self.fs // 1000
        a_n, v = float(rng.uniform(20.0, 27.0)), float(rng.uniform(0.05, 0.6))
        return synth.random_scene(self.fs, self.n_ms, self.n_sats, self.seed, max_code_phase=(2046 if n > 2046 else None),
                                  amplitude=a_n / n, noise_sigma=float(np.sqrt(v / n)))

    def build(self) -> Tuple[np.ndarray, List[int], int]:
        """(iq, search list, X's satellite id)."""
        scene = self.scene()
        x = scene.sats[0].sat_id
        mask = np.ones(self.n_ms, dtype=np.int8)
        mask[self.absent_ms[0]:self.absent_ms[1]] = 0
        present = {s.sat_id for s in scene.sats}
        absent = [sv for sv in range(1, 33) if sv not in present][:self.n_absent_on_list]
        return render_with_presence(scene, {x: mask}), sorted(present | set(absent)), x


# The seeds were chosen with the float64 model on a CPU (seed_search below: the first seed that meets every condition of
# scene_conditions).  Smallest margins the model recorded with them, against the bounds below (1e-4, 1e-3, 1e-3, 1e-3):
#        relative lock margin   |circularity - 0.2|   |circularity - 0.93|   |strength - threshold|
#   R1        1.08e-4                 0.168                 0.069                  0.38
#   R2        1.02e-4                 0.119                 0.047                  0.75
#   R3        7.7e-4                  0.019                 0.045                  0.47
# The lock margins of R1 and R2 clear their bound by 8 % and 2 % only: the smallest of some 37 000 and 9 500 lock comparisons lies
# near 1e-4 for most seeds.  A change to synth.render or to the oracle's tracker moves them, and scene_conditions then names the
# margin that fell short; the remedy is a new seed from seed_search and new figures here, never a lower bound.
R1 = LifecycleScene("R1", 2_046_000, 10_300, 4, seed=33, absent_ms=(2500, 8000), n_absent_on_list=2, scan_period_s=10, watchdog_period_s=6)
R2 = LifecycleScene("R2", 2_046_000, 3_500, 3, seed=7, absent_ms=(700, 2200), n_absent_on_list=0, scan_period_s=1, watchdog_period_s=0.6)
R3 = LifecycleScene("R3", 8_184_000, 3_500, 3, seed=38, absent_ms=(700, 2200), n_absent_on_list=0, scan_period_s=1, watchdog_period_s=0.6)

MIN_LOCK_MARGIN = 1e-4            # relative, orc.lock_margins
MIN_CIRCULARITY_MARGIN = 1e-3     # from 0.2 and from 0.93
MIN_STRENGTH_MARGIN = 1e-3        # from the acquisition threshold


def scene_conditions(model, x: int) -> List[str]:
    """What is wrong with a finished model run as a leave-and-return scene; empty when every condition holds."""
    bad = []
    lives = model.lives.get(x, [])
    if len(lives) < 2:
        return [f"X = {x} has {len(lives)} lives"]
    first, second = lives[0], lives[1]
    if first.lost_at is None or not first.looks or first.looks[-1].action != "drop" or first.looks[-1].step != first.lost_at:
        bad.append("X's first life does not end in a watchdog drop")
    rescans = [sc for sc in model.scans if sc.step == second.acquired_at and x in sc.acquired and sc.step > (first.lost_at or 0)]
    if not rescans:
        bad.append("X is not acquired again by a later scan")
    look = second.looks[0] if second.looks else None
    if look is None or look.step != second.acquired_at or look.n_peaks != 1 or look.circularity is not None or look.action != "none":
        bad.append(f"the first look of X's second life is {look}")
    if len(second.records) < 250:
        bad.append(f"X's second life runs {len(second.records)} ms")
    others = [life for sv, ls in model.lives.items() if sv != x for life in ls]
    if not any(sum(r.locked for r in life.records) > len(life.records) / 2 for life in others):
        bad.append("no other satellite is locked for more than half of its milliseconds")
    if any(len(ls) != 1 or ls[0].lost_at is not None or ls[0].acquired_at != 9 for sv, ls in model.lives.items() if sv != x):
        bad.append("another satellite is dropped or acquired late: the scan schedule would not be the scene's")
    if len(lives) != 2 or second.lost_at is not None:
        bad.append("X is lost a second time")
    m = model.margins()
    if not m["lock"] > MIN_LOCK_MARGIN:
        bad.append(f"lock margin {m['lock']:.3e}")
    if not (m["circularity_drop"] >= MIN_CIRCULARITY_MARGIN and m["circularity_nudge"] >= MIN_CIRCULARITY_MARGIN):
        bad.append(f"circularity margins {m['circularity_drop']:.3e} / {m['circularity_nudge']:.3e}")
    if not m["strength"] >= MIN_STRENGTH_MARGIN:
        bad.append(f"strength margin {m['strength']:.3e}")
    return bad


def run_model(spec: LifecycleScene, iq, search: List[int], pool=None):
    """The float64 receiver model over a scene, with the scene's two periods patched in for the run (and restored)."""
    import receiver_model as rm

    old = (rm.ACQUISITION_SCAN_FREQUENCY, orc.WATCHDOG_PERIOD_S)
    rm.ACQUISITION_SCAN_FREQUENCY, orc.WATCHDOG_PERIOD_S = spec.scan_period_s, spec.watchdog_period_s
    try:
        return rm.ReceiverModel(iq, spec.fs, search, n_steps=spec.n_ms, pool=pool).run()
    finally:
        rm.ACQUISITION_SCAN_FREQUENCY, orc.WATCHDOG_PERIOD_S = old


def seed_search(spec: LifecycleScene, seeds, pool=None) -> Optional[int]:
    """The first of `seeds` whose scene meets every condition in the model (how the seeds above were found)."""
    for seed in seeds:
        cand = dataclasses.replace(spec, seed=seed)
        iq, search, x = cand.build()
        model = run_model(cand, iq, search, pool)
        bad = scene_conditions(model, x)
        print(f"{spec.name} seed {seed}: {bad or 'ok'} {model.margins()}", flush=True)
        if not bad:
            return seed
    return None
