"""The run-time switches of the library (include/aqc_switches.def): ``python -m aqc_research_amd.switches`` prints the table."""
from ctypes import byref, c_char_p
from typing import Dict, List

from ._lib import lib


def table() -> List[Dict[str, str]]:
    """One dict per switch: name, default, when (import / create / call), reader (c / python), doc."""
    rows, fields = [], [c_char_p() for _ in range(5)]
    while lib().aqc_switch_info(len(rows), *map(byref, fields)) == 0:
        rows.append(dict(zip(("name", "default", "when", "reader", "doc"), (f.value.decode() for f in fields))))
    return rows


if __name__ == "__main__":
    for row in table():
        print("{name}  default {default}, read at {when} by {reader}\n    {doc}".format(**row))
