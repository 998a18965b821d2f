/* Stand-in for <windows.h>: the three names the reference's headers mention (Camera3D.h, PrintMachine.h). */
#pragma once
typedef void* HANDLE;
typedef short SHORT;
struct COORD {
    SHORT X;
    SHORT Y;
};
