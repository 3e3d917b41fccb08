"""The host side every field output shares: the sample schedule, the observers of the regions, the file and the resume.

    class FieldSpectrum(FieldOutput)      spectra.py        one engine.Accumulator per region
    class FieldDecay(FieldOutput)         decay.py          one engine.BandAccumulator
    class FieldDirectional(FieldOutput)   directional.py    one engine.VectorBandAccumulator
    class FieldRecording(FieldOutput)     recordings.py     one engine.DecimatingRecorder or engine.VectorDecimatingRecorder
    class FieldWriter(Schedule)           fields.py         no observer: frames through the host
    class WallAbsorption(FieldOutput)     absorption.py     one engine.Absorption, no regions: it reads the walls

The rules, for all device-side kinds:
  * Samples are due at the steps first, first + every, ... below Nt (Schedule); `every` is 1 for every kind but the spectrum -- a recursive filter
    over skipped samples is another filter.  The sample of step n is u^n, the field the receivers of step n sample.
  * `take(obj, n)` takes the sample of step n and of no other: a sample is NEVER shifted.  A chain answers only while no slab is inside a pair or
    a triple (PfError.code == 4 there), so a chain that is sampled is created with PF_MULTI_NO_PAIRS | PF_MULTI_NO_TRIPLES; take says so.
  * `attach(obj)` makes one observer per region on obj (a HipEngine or a HipMulti) -- `accs` or `recs` --; take attaches by itself.
  * `write()` writes the file as it stands to a temporary name and moves it into place with os.replace: a reader never sees half of it.
  * With resume_at (the step a resumed run continues at) the file must exist and hold the output of the same regions, Ts, first and whatever else
    the kind lists, and its count must be the number of sample steps below resume_at; otherwise it is refused with the field's name.  The file
    keeps the raw state beside the scaled output; attach sets it into the new observers and the run goes on to the file of a run in one piece.

A kind gives: `label`, `noun`, `holds`, `observers_noun` (the words of the messages), `_observer` (one observer for a region), `_restore_observer`
(one observer's saved state), `_sample` (the arguments of every observer's add at step n), `_write_head` and `_write_region`, `_read_file`,
`_checks` (the fields a resumed file must match, in the order they are reported) and `_saved` (what attach restores).
"""
import os

import numpy as np

from .engine import PfError


class Schedule:
    """the sample steps first, first + every, ... below sd.Nt"""
    every = 1

    def next_step(self, n):
        """the first step >= n at which a sample is due (it may lie at or past Nt: no sample then)"""
        return self.first if n <= self.first else self.first + -(-(n - self.first) // self.every) * self.every

    def due(self, n):
        return n < self.sd.Nt and self.next_step(n) == n

    def samples_below(self, n):
        """how many sample steps lie below step n"""
        return 0 if n <= self.first else -(-(n - self.first) // self.every)


def normalise_regions(regions):
    """[(lo, hi, stride)] of anything int-like -> (the same in tuples of int, the file's table int64 [R, 9])"""
    regions = [tuple(tuple(int(v) for v in t) for t in r) for r in regions]
    return regions, np.array([lo + hi + st for lo, hi, st in regions], dtype=np.int64).reshape(-1, 9)


class FieldOutput(Schedule):
    label = noun = holds = observers_noun = None  # "field spectrum", "spectra", "sums", "accumulators": the kind's words in the messages

    def __init__(self, path, sd, regions, first):
        self.path, self.sd = os.fspath(path), sd
        self.regions, self.table = normalise_regions(regions)
        self.first, self.Ts = int(first), float(sd.Ts)
        self.observers, self._restore = None, None

    def _resume(self, resume_at):
        """the last line of a kind's __init__: the file's state is kept for attach"""
        if resume_at is not None:
            self._restore = self._read_matching(int(resume_at))

    # ---- the observers ----
    def attach(self, obj):
        """one observer per region on obj (a HipEngine or a HipMulti); a resumed run's state goes into them"""
        if self.observers is not None:
            return
        self.observers = self._observers(obj)
        if self._restore is not None:
            for i, o in enumerate(self.observers):
                self._restore_observer(o, i, *self._restore)
            self._restore = None

    def _observers(self, obj):
        """one per region; a kind without regions (absorption.py) makes its own"""
        return [self._observer(obj, lo, hi, st) for lo, hi, st in self.regions]

    def settle(self, obj, n):
        """before a write with obj standing before step n: nothing to do for a kind whose sample of step n belongs to step n (absorption.py closes step n - 1)"""

    @property
    def count(self):
        if self.observers is None:
            return self._restore[0] if self._restore is not None else 0
        return self.observers[0].count

    def _due_rule(self):
        return f"first {self.first}"

    def _before_sample(self):
        pass

    def take(self, obj, n):
        """the sample of step n (due(n)) -- never of another step"""
        if not self.due(n):
            raise ValueError(f"{type(self).__name__}.take: no sample is due at step {n} ({self._due_rule()}, Nt {self.sd.Nt})")
        self.attach(obj)
        self._before_sample()
        args = self._sample(n)
        try:
            for o in self.observers:
                o.add(*args)
        except PfError as e:
            if e.code != 4:  # (PF_ERR_STATE: a slab inside a pair or triple; no slab took the sample)
                raise
            err = PfError(f"{self.label}: step {n} cannot be sampled, a slab is inside a blocked pass there, and a sample is never shifted: "
                          f"create the chain with PF_MULTI_NO_PAIRS | PF_MULTI_NO_TRIPLES ({e})")
            err.code = 4
            raise err
        return n

    def _attached(self, what):
        if self.observers is None:
            raise ValueError(f"{type(self).__name__}.{what}: no {self.observers_noun} yet (attach or take first)")

    def write(self):
        """the file as it stands: every region's output and state so far"""
        self._attached("write")
        tmp = self.path + ".tmp"
        self._write_head(tmp, append=False)
        for i, o in enumerate(self.observers):
            self._write_region(tmp, i, o)
        os.replace(tmp, self.path)

    def close(self):
        for o in self.observers or []:
            o.close()
        self.observers = None

    # ---- the file of a resumed run ----
    def _same_clock(self, f):
        """the checks of Ts and first, as rows of `_checks`"""
        return [("Ts", f["Ts"] == self.Ts, f"{f['Ts']!r} in the file, {self.Ts!r} in the scene"), self._asked("first", f["sampling"][0], self.first)]

    @staticmethod
    def _asked(field, theirs, mine, note=""):
        return field, int(theirs) == mine, f"{int(theirs)} in the file, {mine} asked for{note}"

    def _other(self, f, field, what=None):
        """a row of `_checks`: the file's array `field` is mine"""
        return field, np.array_equal(f[field], getattr(self, field)), f"the file holds the {self.holds} of other {what or field}"

    def _read_matching(self, resume_at):
        """what attach restores -- (count, ...) -- from the file a resumed run continues, or ValueError naming the field that differs"""
        if not os.path.exists(self.path):
            raise ValueError(f"{self.path}: no {self.noun} file to resume from")
        f = self._read_file()
        count, below = int(f["sampling"][2]), self.samples_below(resume_at)
        rows = [("regions", np.array_equal(f["regions"], self.table), f"the file holds the {self.holds} of other regions")] + self._checks(f)
        for field, same, text in rows + [("count", count == below, f"the file holds {count} samples, {below} sample steps lie below step {resume_at}")]:
            if not same:
                raise ValueError(f"{self.path}: {field}: {text}")
        return self._saved(f, count)
