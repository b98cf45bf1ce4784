/* Stand-in for the console calls the reference's render loop makes between buckets
 * (it polls for an Esc key press).  Here no key is ever pending.  Our own text. */
#ifndef MRT_REF_WINDOWS_SHIM_H
#define MRT_REF_WINDOWS_SHIM_H

typedef void* HANDLE;
typedef unsigned long DWORD;
struct MRT_REF_KEY_EVENT { unsigned short wVirtualKeyCode; };
struct INPUT_RECORD { struct { MRT_REF_KEY_EVENT KeyEvent; } Event; };
enum { STD_INPUT_HANDLE = -10, VK_ESCAPE = 0x1B };

static inline HANDLE GetStdHandle(int) { return 0; }
static inline int FlushConsoleInputBuffer(HANDLE) { return 1; }
static inline int PeekConsoleInput(HANDLE, INPUT_RECORD*, DWORD, DWORD* n) { *n = 0; return 1; }
static inline int ReadConsoleInput(HANDLE, INPUT_RECORD*, DWORD, DWORD* n) { *n = 0; return 1; }

#endif
