# The two numbers of the C ABI that the tests hold independently of include/b4c.h: adding an entry point changes ENTRY_POINTS here.
ABI_VERSION = 13
ENTRY_POINTS = 150
