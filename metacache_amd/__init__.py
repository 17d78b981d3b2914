def __getattr__(name):            # the public calls live in metacache_amd.api; importing the package alone loads nothing
    if name in ("align_semiglobal", "Aligner"):
        from . import api
        return getattr(api, name)
    raise AttributeError(name)
