// Windows.h stand-in — TEST INFRASTRUCTURE ONLY (oracle/ref/). The Win32 type names the reference's
// headers mention; nothing here does anything.
#pragma once
#include <cstddef>
#include <cstdint>

typedef unsigned int UINT;
typedef uint8_t UINT8;
typedef uint16_t UINT16;
typedef uint32_t UINT32;
typedef uint64_t UINT64;
typedef int INT;
typedef int BOOL;
typedef uint32_t DWORD;
typedef int32_t LONG;
typedef int32_t HRESULT;
typedef float FLOAT;
typedef char* LPSTR;
typedef const char* LPCSTR;
typedef const wchar_t* LPCWSTR;
typedef void* HANDLE;
typedef void* HINSTANCE;
typedef void* HWND;
typedef intptr_t LRESULT;
typedef uintptr_t WPARAM;
typedef intptr_t LPARAM;
typedef size_t SIZE_T;

#define CALLBACK
#define WINAPI
#ifndef TRUE
#define TRUE 1
#define FALSE 0
#endif
#define S_OK ((HRESULT)0)
#define FAILED(hr) (((HRESULT)(hr)) < 0)
#define SUCCEEDED(hr) (((HRESULT)(hr)) >= 0)

inline DWORD GetLastError() { return 0; }
