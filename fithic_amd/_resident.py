"""What the objects that hold contact columns resident in HBM have in common (validpairs.ValidPairs, fragpairs.FragPairs,
coarsen.Coarsened, juicer.JuicerContacts, hicpro.HicPro): they own one native handle of _capi with five int32 columns
(chr1, locus1, chr2, locus2, count), close it, fetch the columns and hand them to an Engine from HBM to HBM."""


def _is_gzip(path):
    with open(path, "rb") as f:
        return f.read(2) == b"\x1f\x8b"


class Resident:
    """`names`: the chromosome names the chr columns index.  A subclass names the handle's fetch method in _FETCH and loads what
    its data set holds beside the contacts in _load_tables."""
    _FETCH = "fetch_cells"

    def __init__(self, handle, n, names):
        self._handle, self._n, self.names = handle, n, names

    def close(self):
        if self._handle is not None:
            self._handle.close()
            self._handle = None

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    def __len__(self):
        return self._n

    def counts(self):
        """the native handle's counts of the last call, by name"""
        return self._handle.counts()

    def stage_seconds(self):
        return self._handle.stage_seconds()

    def contacts(self):
        """(chr1, locus1, chr2, locus2, count) fetched from the device; the chr columns index `names`"""
        return getattr(self._handle, self._FETCH)()

    def intern(self, chroms):
        """these names into the run's ChromIndex: empty (it receives them) or one whose ids agree with them.  Call it before the
        fragments are interned when those are loaded first (fragments.bins)."""
        for k, name in enumerate(self.names):
            if chroms.intern(name) != k:
                raise ValueError("chromosome %r has id %d in the given ChromIndex and %d here" % (name, chroms.intern(name), k))

    def _load_tables(self, engine, chroms):
        """the fragments (and bias) of a data set that brings its own; the others go into an Engine whose fragments are loaded"""

    def load_into(self, engine, chroms):
        """The data set into a configured Engine; the five columns go from HBM to HBM."""
        self.intern(chroms)
        self._load_tables(engine, chroms)
        engine.load_contacts_device(self._handle.device_ptrs() if self._n else [0] * 5, self._n, self._handle.stream())
        engine.ctx.sync()                                            # the engine has its own copy: this object may be closed now
