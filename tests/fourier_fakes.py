"""CPU stand-in for the first-layer kind of nsfnet_amd.engine.DeviceNet (TEST INFRASTRUCTURE), on top of any of the
other fakes: the stand-in net has no C handle, so it records the kind where the real one asks the library (and refuses
what the library refuses).  The stand-in plans keep the tanh arithmetic of their base: these fakes serve the host logic
around the option - initialisation, sidecars, fingerprints - not its numbers.  Nothing here is reachable from the
product path."""
import state_fakes
from nsfnet_amd import engine as eng


def install(monkeypatch=None, base=state_fakes):
    """base.install plus a DeviceNet that keeps the first-layer kind on the host."""
    base.install(monkeypatch)

    class FourierDeviceNet(eng.DeviceNet):
        def set_first_layer(self, kind):
            if int(kind) not in (0, 1):
                raise ValueError("kind must be 0 or 1")
            if int(kind) == 1 and (self.hidden % 2 or self.n_hidden < 2):
                raise ValueError("frozen sine layer: even hidden width and at least 2 hidden layers")
            self.first_layer = int(kind)

    if monkeypatch is not None:
        monkeypatch.setattr(eng, "DeviceNet", FourierDeviceNet)
    else:
        eng.DeviceNet = FourierDeviceNet
