"""What this node's kfd offers, asked of the driver itself (for tests whose
subject is one of these facilities)."""
from __future__ import annotations

import errno
import fcntl
import os
import struct

KFD_PROC_DIR = "/sys/class/kfd/kfd/proc"
# AMDKFD_IOC_SMI_EVENTS = _IOWR('K', 0x1F, struct kfd_ioctl_smi_events_args {u32 gpuid; u32 anon_fd;})
_AMDKFD_IOC_SMI_EVENTS = (3 << 30) | (8 << 16) | (ord("K") << 8) | 0x1F


def kfd_process_list_present(proc_dir: str = KFD_PROC_DIR) -> bool:
    """kfd lists its processes and their queues under sysfs (a guest's kfd may not)."""
    return os.path.isdir(proc_dir)


def kfd_smi_events_refused(gpu_id: int, dev_kfd: str = "/dev/kfd") -> str:
    """"" when kfd hands out an SMI event descriptor for `gpu_id` (what
    amd-smi's event notification subscribes through), else why not."""
    try:
        fd = os.open(dev_kfd, os.O_RDWR | os.O_CLOEXEC)
    except OSError as e:
        return f"{dev_kfd}: {e}"
    try:
        out = fcntl.ioctl(fd, _AMDKFD_IOC_SMI_EVENTS, struct.pack("II", gpu_id, 0))
        os.close(struct.unpack("II", out)[1])
        return ""
    except OSError as e:
        return f"AMDKFD_IOC_SMI_EVENTS: {errno.errorcode.get(e.errno, e.errno)} ({e.strerror})"
    finally:
        os.close(fd)


def kfd_holders(dev_kfd: str = "/dev/kfd") -> list:
    """PIDs (as strings) of the processes this one can see holding `dev_kfd`
    open: where kfd lists no processes, the GPU processes there are."""
    out = []
    for pid in os.listdir("/proc"):
        if not pid.isdigit():
            continue
        try:
            if any(os.readlink(f"/proc/{pid}/fd/{fd}") == dev_kfd for fd in os.listdir(f"/proc/{pid}/fd")):
                out.append(pid)
        except OSError:
            continue
    return sorted(out)
