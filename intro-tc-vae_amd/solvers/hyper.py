"""The two validating descriptors behind every solver hyperparameter.  Both take their name from ``__set_name__``, check
on every assignment, store under ``obj.__dict__["_" + name]`` and return themselves on class-level access.  The values
are scalar kernel arguments or kernel selectors frozen into a captured step, so each solver puts them into its
``_graph_key_extra()``: a change re-captures."""
import math
import numbers


class Choice:
    """One of ``options``; ``default`` is read until the first assignment."""

    def __init__(self, options, default):
        self.options, self.default = tuple(options), default

    def __set_name__(self, owner, name):
        self.name = name

    def __get__(self, obj, cls=None):
        return self if obj is None else obj.__dict__.get("_" + self.name, self.default)

    def __set__(self, obj, value):
        if value not in self.options:
            raise ValueError(f"{self.name} must be one of {self.options} (got {value!r})")
        obj.__dict__["_" + self.name] = value


class Number:
    """A finite ``numbers.Real`` that is not a ``bool``, >= 0 (``positive``: > 0), stored as a ``float``.  ``optional``:
    None is accepted and stored; while it is, a read gives ``fallback(obj)`` (no ``fallback``: None)."""

    def __init__(self, positive=False, optional=False, fallback=None):
        self.positive, self.optional, self.fallback = positive, optional, fallback

    def __set_name__(self, owner, name):
        self.name = name

    def __get__(self, obj, cls=None):
        if obj is None:
            return self
        v = obj.__dict__.get("_" + self.name)
        return self.fallback(obj) if v is None and self.fallback is not None else v

    def __set__(self, obj, value):
        if not (value is None and self.optional):
            bad = isinstance(value, bool) or not isinstance(value, numbers.Real) or not math.isfinite(value)
            if bad or value < 0 or (self.positive and value == 0):
                raise ValueError(f"{self.name} must be a finite number {'> 0' if self.positive else '>= 0'}"
                                 f"{' or None' if self.optional else ''} (got {value!r})")
            value = float(value)
        obj.__dict__["_" + self.name] = value
