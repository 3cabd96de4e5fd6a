"""forced_routes: entries of gen6d_amd.network.refiner.ROUTES set for the duration of a block — how the route tests force a layer onto a
kernel.  Networks made inside the block pack their filters for the forced table; the table is put back as it was."""
import contextlib

from gen6d_amd.network import refiner

PAIR_KEYS = {net.name: tuple(k for k in refiner.ROUTES if k.startswith(net.name + ".") and "pair" in refiner.ROUTES[k])
             for net in (refiner.FEATNET, refiner.VOLUME)}


def igemm_layers(routes=None):
    """{layer: loader variant} of the layers `routes` (default: the product's table) puts on the implicit-GEMM pair mode."""
    routes = refiner.ROUTES if routes is None else routes
    return {k: int(r[5:]) for k, rs in routes.items() for r in rs if r.startswith("igemm")}


def with_pairs(keys):
    """Entries that put the layers `keys` on the pair kernel (in front of whatever they list)."""
    return {k: ("pair",) + tuple(r for r in refiner.ROUTES.get(k, ()) if r != "pair") for k in keys}


def without(route, keys=None):
    """Entries that take the routes named `route` ("pair" / "igemm": every variant) off `keys` (default: every layer)."""
    return {k: tuple(r for r in rs if not r.startswith(route)) for k, rs in refiner.ROUTES.items() if keys is None or k in keys}


@contextlib.contextmanager
def forced_routes(entries):
    saved = dict(refiner.ROUTES)
    refiner.ROUTES.update(entries)
    try:
        yield
    finally:
        refiner.ROUTES.clear()
        refiner.ROUTES.update(saved)
